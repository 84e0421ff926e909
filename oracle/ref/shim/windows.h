/*
 * oracle/ref/shim/windows.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Stand-in for <windows.h>, written for this repository: just the names the
 * reference's viterbi.h, deconvolve.cpp and rschecksf.cpp mention when they
 * are compiled with -D_VIT_NO_ASM_ and without the logging options.  None of
 * the Win32 API is provided; the decoders and the RS checker call none of it.
 */
#ifndef VITREF_SHIM_WINDOWS_H
#define VITREF_SHIM_WINDOWS_H

#include <stdint.h>

typedef uint64_t DWORD64;
typedef uint32_t DWORD;
typedef int32_t LONG;
typedef int64_t LONG64;
typedef int BOOL;
typedef unsigned char BOOLEAN;
typedef void *PVOID;
typedef void *HANDLE;

#define MAX_PATH 260
#define WINAPI
#define UNREFERENCED_PARAMETER(x) ((void)(x))

#endif
