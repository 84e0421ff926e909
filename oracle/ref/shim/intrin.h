/*
 * oracle/ref/shim/intrin.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Stand-in for MSVC's <intrin.h>: the x86 vector intrinsics, and the `min`
 * macro that <windows.h> normally supplies (rschecksf.cpp uses it).  The macro
 * comes AFTER the include: the C++ library's configuration header removes a
 * `min` macro that is defined before it.
 */
#ifndef VITREF_SHIM_INTRIN_H
#define VITREF_SHIM_INTRIN_H

#include <immintrin.h>

#ifndef min
#define min(a, b) (((a) < (b)) ? (a) : (b))
#endif

#endif
