/*
 * oracle/ref/harness.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Written for this repository; it contains no text of the reference.  It is
 * linked with the reference's own deconvolve.cpp and rschecksf.cpp (compiled in
 * place from a reference checkout, see oracle/ref.py) into
 * oracle/_ref/libvitref.so, and provides
 *
 *   - what those two translation units import from the rest of the DLL (which is
 *     Windows start-up code and MASM data and is not built): the decoder's
 *     vector constants, symbols32LUT, rsLUT, deconJumpTarget;
 *   - a plain C interface (`ref_*`) for ctypes.
 *
 * The Galois-field tables are built here from the field's definition
 * (GF(2^8), x^8+x^4+x^3+x^2+1, alpha = x), not taken from the DLL's start-up
 * code: they are the one part of the RS path that this build does NOT pin.
 *
 * No C++ run-time library is used (no new/delete, no exceptions, no iostream):
 * the shared object depends on libc and libpthread only.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef REF_RENORM_THRESHOLD
#define REF_RENORM_THRESHOLD 150 /* what oracle/ref.py put into the build's viterbi.h; reported by ref_renorm_threshold() */
#endif

#define REF_MAXBITS 9216 /* the decoders keep 9216 + 6 decision words on their stack */

/* ---- the decoders' constants -------------------------------------------------
 * One trellis step handles 32 butterflies; byte i of a mask is 0xFF where the
 * code polynomial of that output symbol taps state 2i.  The 128-bit decoders
 * hold butterflies 0..15 and 16..31 in two registers (symbols 0 and 3 share a
 * polynomial, hence "1st"/"2nd"); the 256-bit decoders hold all 32 with the two
 * middle quadwords exchanged.  The byte values are data of the reference
 * (const.asm); tests/test_ref_parity.py derives them again from the polynomials. */
#define Z 0x00
#define F 0xFF
extern "C" {
extern const unsigned char m256_63_0[32], m128_63_0[16], m128_63[16], m128_1st_XOR_0_3_4_7[16], m128_2nd_XOR_0_3_4_7[16],
    m128_XOR_1_5[16], m128_XOR_2_6[16], m128_16X_0x1[16], m256_XOR_0_3_4_7[32], m256_XOR_1_5[32], m256_XOR_2_6[32];
alignas(64) const unsigned char m256_63_0[32] = {0,  63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63,
                                                 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};
alignas(16) const unsigned char m128_63_0[16] = {0, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};
alignas(16) const unsigned char m128_63[16] = {63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};
alignas(16) const unsigned char m128_1st_XOR_0_3_4_7[16] = {Z, Z, F, F, F, F, Z, Z, Z, Z, F, F, F, F, Z, Z};
alignas(16) const unsigned char m128_2nd_XOR_0_3_4_7[16] = {F, F, Z, Z, Z, Z, F, F, F, F, Z, Z, Z, Z, F, F};
alignas(16) const unsigned char m128_XOR_1_5[16] = {Z, F, F, Z, F, Z, Z, F, Z, F, F, Z, F, Z, Z, F};
alignas(16) const unsigned char m128_XOR_2_6[16] = {Z, F, Z, F, Z, F, Z, F, F, Z, F, Z, F, Z, F, Z};
alignas(16) const unsigned char m128_16X_0x1[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
alignas(32) const unsigned char m256_XOR_0_3_4_7[32] = {Z, Z, F, F, F, F, Z, Z, F, F, Z, Z, Z, Z, F, F,
                                                        Z, Z, F, F, F, F, Z, Z, F, F, Z, Z, Z, Z, F, F};
alignas(32) const unsigned char m256_XOR_1_5[32] = {Z, F, F, Z, F, Z, Z, F, Z, F, F, Z, F, Z, Z, F,
                                                    Z, F, F, Z, F, Z, Z, F, Z, F, F, Z, F, Z, Z, F};
alignas(32) const unsigned char m256_XOR_2_6[32] = {Z, F, Z, F, Z, F, Z, F, Z, F, Z, F, Z, F, Z, F,
                                                    F, Z, F, Z, F, Z, F, Z, F, Z, F, Z, F, Z, F, Z};

/* the SSE2 decoder's broadcast table: entry i = byte i in all four bytes */
int *symbols32LUT;
}
#undef Z
#undef F

/* ---- what the two translation units import / export with C++ linkage ------------ */
typedef int DECON(unsigned int, unsigned int *, int, unsigned char *);
DECON *deconJumpTarget;

struct RS_LookUp { /* layout of viterbi.h: 768 antilogs (index mod 255 unrolled three times), 256 logs */
    unsigned char RS_ato_mod[768];
    unsigned char RS_iof[256];
};
RS_LookUp *rsLUT;

extern "C" {
DECON decon_sse2_lut32, decon_ssse3, decon_avx, decon_avx2, decon_avx5;
}
int deconvolve(unsigned int framebits, unsigned int *piData, int inputLength, unsigned char *output);
int RScheckSuperframe(unsigned char *p, int startIx, unsigned int RSDims, unsigned char *outVector);
int DECODE_RS(unsigned int *data, unsigned char *ato_mod, unsigned char *index_of);

/* ---- CPU features (cpuid directly: no dependence on a compiler run-time) -------- */
enum { REF_SSE2 = 1, REF_SSSE3 = 2, REF_AVX = 4, REF_AVX2 = 8, REF_AVX5 = 16 };

static void ref_cpuid(unsigned leaf, unsigned sub, unsigned r[4]) {
    __asm__ volatile("cpuid" : "=a"(r[0]), "=b"(r[1]), "=c"(r[2]), "=d"(r[3]) : "a"(leaf), "c"(sub));
}
static unsigned long long ref_xcr0(void) {
    unsigned lo, hi;
    __asm__ volatile("xgetbv" : "=a"(lo), "=d"(hi) : "c"(0));
    return ((unsigned long long)hi << 32) | lo;
}
static int ref_detect(void) {
    unsigned r[4], f = 0;
    ref_cpuid(0, 0, r);
    unsigned maxleaf = r[0];
    ref_cpuid(1, 0, r);
    if (r[3] & (1u << 26)) f |= REF_SSE2;
    if (r[2] & (1u << 9)) f |= REF_SSSE3;
    unsigned long long xcr = (r[2] & (1u << 27)) ? ref_xcr0() : 0; /* OSXSAVE: the OS keeps the wide registers */
    int ymm = (xcr & 0x6) == 0x6, zmm = (xcr & 0xE6) == 0xE6;
    if ((r[2] & (1u << 28)) && ymm) f |= REF_AVX;
    if (maxleaf >= 7) {
        ref_cpuid(7, 0, r);
        if ((f & REF_AVX) && (r[1] & (1u << 5))) f |= REF_AVX2;
        if ((f & REF_AVX2) && zmm && (r[1] & (1u << 16)) && (r[1] & (1u << 30)) && (r[1] & (1u << 31))) f |= REF_AVX5;
    }
    return (int)f;
}

/* ---- set-up -------------------------------------------------------------------- */
static RS_LookUp g_lut;
static int g_sym_lut[256];
static int g_features;

__attribute__((constructor)) static void ref_setup(void) {
    /* antilog / log over GF(2^8) modulo 0x11D, alpha = 2 */
    unsigned char pw[255];
    unsigned x = 1;
    g_lut.RS_iof[0] = 255; /* log 0: the "no term" marker */
    for (int i = 0; i < 255; i++) {
        pw[i] = (unsigned char)x;
        g_lut.RS_iof[x] = (unsigned char)i;
        x <<= 1;
        if (x & 0x100) x ^= 0x11D;
    }
    for (int i = 0; i < 768; i++) g_lut.RS_ato_mod[i] = pw[i % 255];
    for (int i = 0; i < 256; i++) g_sym_lut[i] = (int)(0x01010101u * (unsigned)i);
    rsLUT = &g_lut;
    symbols32LUT = g_sym_lut;
    g_features = ref_detect();
    deconJumpTarget = decon_sse2_lut32;
}

/* ---- the C interface ------------------------------------------------------------- */
#define REF_NVARIANTS 5
static DECON *const g_variant[REF_NVARIANTS] = {decon_sse2_lut32, decon_ssse3, decon_avx, decon_avx2, decon_avx5};
static const int g_need[REF_NVARIANTS] = {REF_SSE2, REF_SSE2 | REF_SSSE3, REF_AVX, REF_AVX2, REF_AVX5};

static int ref_usable(int variant) {
    return variant >= 0 && variant < REF_NVARIANTS && (g_features & g_need[variant]) == g_need[variant];
}
/* The 128-bit C decoders store each 16-bit decision mask as a 32-bit int through a pointer that advances by 16 bits, so
 * their last store reaches 2 bytes past the decision array when the frame fills it (framebits == 9216, the ABI's
 * maximum): a write outside the function's own stack frame, whose effect depends on the caller.  The 256-bit decoders
 * store whole ints and stay inside.  The harness does not make that call. */
static unsigned ref_maxbits(int variant) { return variant <= 2 ? REF_MAXBITS - 2 : REF_MAXBITS; }

extern "C" {

int ref_cpu_features(void) { return g_features; }
int ref_variant_supported(int variant) { return ref_usable(variant); }
int ref_renorm_threshold(void) { return REF_RENORM_THRESHOLD; }
unsigned ref_max_framebits(int variant) { return ref_usable(variant) ? ref_maxbits(variant) : 0; }

/* one frame, reference ABI (one u32 per soft symbol, 4*(framebits+6) of them).  -2: variant not usable on this CPU,
 * -3: a length the variant's stack array cannot hold.  Otherwise the decoder's own return value. */
int ref_decon(int variant, unsigned framebits, unsigned *symbols, unsigned char *out) {
    if (!ref_usable(variant)) return -2;
    if (framebits > ref_maxbits(variant)) return -3;
    return g_variant[variant](framebits, symbols, 0, out);
}
int ref_decon_sse2_lut32(unsigned fb, unsigned *s, unsigned char *o) { return ref_decon(0, fb, s, o); }
int ref_decon_ssse3(unsigned fb, unsigned *s, unsigned char *o) { return ref_decon(1, fb, s, o); }
int ref_decon_avx(unsigned fb, unsigned *s, unsigned char *o) { return ref_decon(2, fb, s, o); }
int ref_decon_avx2(unsigned fb, unsigned *s, unsigned char *o) { return ref_decon(3, fb, s, o); }
int ref_decon_avx5(unsigned fb, unsigned *s, unsigned char *o) { return ref_decon(4, fb, s, o); }

/* the DLL's exported entry: the dispatcher through deconJumpTarget (not thread safe here: it sets the target) */
int ref_deconvolve(int variant, unsigned framebits, unsigned *symbols, unsigned char *out) {
    if (!ref_usable(variant)) return -2;
    if (framebits > ref_maxbits(variant)) return -3;
    deconJumpTarget = g_variant[variant];
    return deconvolve(framebits, symbols, 0, out);
}

struct ref_job {
    int variant;
    unsigned framebits;
    const uint8_t *sym;
    unsigned char *out;
    long f0, f1;
    int rc;
};

static void *ref_worker(void *p) {
    ref_job *j = (ref_job *)p;
    size_t ssz = 4u * (j->framebits + 6), osz = (j->framebits + 7) / 8;
    unsigned *wide = (unsigned *)malloc(ssz * sizeof(unsigned));
    if (!wide) {
        j->rc = -4;
        return 0;
    }
    for (long f = j->f0; f < j->f1; f++) {
        const uint8_t *s = j->sym + ssz * (size_t)f;
        for (size_t i = 0; i < ssz; i++) wide[i] = s[i];
        int rc = g_variant[j->variant](j->framebits, wide, 0, j->out + osz * (size_t)f);
        if (rc) j->rc = rc;
    }
    free(wide);
    return 0;
}

/* frames contiguous, one BYTE per soft symbol (widened to the reference's u32 here), (framebits+7)/8 output bytes per
 * frame.  Every frame runs on a thread with a 1 MiB stack: a call of a reference decoder keeps 74 KB of decisions there. */
int ref_decode_batch_u8(int variant, unsigned framebits, const uint8_t *symbols, unsigned char *out, long nframes,
                        int nthreads) {
    if (!ref_usable(variant)) return -2;
    if (framebits > ref_maxbits(variant)) return -3;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 1u << 20);
    pthread_t th[64];
    ref_job jobs[64];
    long per = (nframes + nthreads - 1) / nthreads;
    int started = 0, rc = 0;
    for (int i = 0; i < nthreads; i++) {
        long f0 = per * i, f1 = f0 + per > nframes ? nframes : f0 + per;
        if (f0 >= f1) break;
        jobs[i].variant = variant;
        jobs[i].framebits = framebits;
        jobs[i].sym = symbols;
        jobs[i].out = out;
        jobs[i].f0 = f0;
        jobs[i].f1 = f1;
        jobs[i].rc = 0;
        if (pthread_create(&th[i], &attr, ref_worker, &jobs[i]) != 0) {
            rc = -5;
            break;
        }
        started++;
    }
    for (int i = 0; i < started; i++) {
        pthread_join(th[i], 0);
        if (jobs[i].rc) rc = jobs[i].rc;
    }
    pthread_attr_destroy(&attr);
    return rc;
}

int ref_rs_check_superframe(unsigned char *p, int startIx, unsigned RSDims, unsigned char *outVector) {
    return RScheckSuperframe(p, startIx, RSDims, outVector);
}

/* nsf superframes back to back; out is NOT cleared (the caller's sentinel shows what was left unwritten) */
void ref_rs_check_batch(unsigned char *p, unsigned RSDims, unsigned char *out, int *ret, long nsf) {
    for (long s = 0; s < nsf; s++)
        ret[s] = RScheckSuperframe(p + (size_t)s * 120 * RSDims, 0, RSDims, out + (size_t)s * 110 * RSDims);
}

/* n codewords of 120 u32 each (bytes widened, as RScheckSuperframe passes them); patched in place */
void ref_decode_rs_batch(unsigned *data, int *ret, long n) {
    alignas(64) unsigned blk[128];
    memset(blk, 0, sizeof blk);
    for (long w = 0; w < n; w++) {
        memcpy(blk, data + 120 * w, 120 * sizeof(unsigned));
        ret[w] = DECODE_RS(blk, rsLUT->RS_ato_mod, rsLUT->RS_iof);
        memcpy(data + 120 * w, blk, 120 * sizeof(unsigned));
    }
}
int ref_decode_rs(unsigned *data) {
    int rc;
    ref_decode_rs_batch(data, &rc, 1);
    return rc;
}

void ref_tables(unsigned char *ato_mod, unsigned char *index_of) {
    memcpy(ato_mod, g_lut.RS_ato_mod, 768);
    memcpy(index_of, g_lut.RS_iof, 256);
}

} /* extern "C" */
