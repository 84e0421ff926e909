// rs_kernels.hip -- batched RScheckSuperframe for gfx950: RS(120,110) over
// GF(2^8)/0x11D (RS(255,245) shortened by 135, roots alpha^0..alpha^9).
//
// One lane decodes one column (codeword); a 256-thread workgroup takes whole
// superframes so the reference's "stop at the first uncorrectable column"
// rule (rschecksf.cpp:80-88) is a workgroup-local min-reduction.
//
// rs_kernel (RSDims <= 256, the DAB+ range): the workgroup's superframes are copied HBM -> LDS
// -> HBM with 16-byte accesses in their natural layout p[j + k*RSDims] (rschecksf.cpp:75-76: lanes
// of one superframe read consecutive bytes of a row, so the column gather needs no transposition).
// The 1190 multiply-adds of the syndrome loop (rschecksf.cpp:210-219) are replaced by the remainder
// of the codeword modulo the generator polynomial: two conflict-free 16-byte LDS lookups per data byte
// (low and high nibble of x -> x*g_0..x*g_9, see NibTable) instead of nine byte lookups; a zero remainder
// is a clean codeword, otherwise the ten syndromes are the remainder evaluated at alpha^i (same field
// elements as the reference's Horner sums, since g(alpha^i) = 0).  The correction path (rs_correct) is
// entered by a whole wavefront as soon as one of its columns has an error: Berlekamp-Massey on logs,
// locator roots in closed form (degree 1, 2), a wavefront per column (chien_wave) or four positions per
// lookup (chien_quad), Forney.  rs_kernel_wide keeps the transposed-LDS form for RSDims > 256.
//
// Replaces, from scratch: RScheckSuperframe (rschecksf.cpp:65-93), DECODE_RS
// (:199-377), Mod255 (:50-52) and CreateLookupTables (dllmain.cpp:124-146).
#include "rs_dev.h"

namespace {

// General form (used for rsdims > 256).  Workgroup = 256 lanes.  For rsdims <= 256 it takes spb = 256/rsdims
// superframes per pass; for wider superframes it walks the columns in 256-wide chunks, in
// order, and stops after the first chunk that holds a failure.
__global__ __launch_bounds__(RS_THREADS) void rs_kernel_wide(const uint8_t* __restrict__ p, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ ret, uint32_t rsdims,
                                                        long long nsf) {
    __shared__ uint8_t cw[NCW * RS_THREADS];  // [row][lane]
    __shared__ uint8_t ato[ATO_SIZE];
    __shared__ uint8_t iof[256];
    __shared__ uint8_t mulp[(NROOTS + 1) * 256];  // mulp[i][x] = x * alpha^i, i = 0..10
    __shared__ uint8_t qsol[256];
    __shared__ uint32_t step[STEP_TERMS * 256];
    __shared__ int s_minfail[RS_THREADS];
    __shared__ int s_sum[RS_THREADS];
    __shared__ int s_fail[RS_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < ATO_SIZE; i += RS_THREADS) ato[i] = g_gf.ato[i];
    iof[tid] = g_gf.iof[tid];
    qsol[tid] = g_quad.q[tid];
    for (int i = 0; i <= NROOTS; i++) mulp[i * 256 + tid] = tid ? g_gf.ato[g_gf.iof[tid] + i] : 0;
    for (int i = tid; i < STEP_TERMS * 256; i += RS_THREADS) step[i] = g_step.w[i];
    __syncthreads();

    const uint32_t spb = rsdims <= RS_THREADS ? RS_THREADS / rsdims : 1u;  // superframes per pass
    const uint32_t nchunk = rsdims <= RS_THREADS ? 1u : (rsdims + RS_THREADS - 1) / RS_THREADS;
    const long long ngroups = (nsf + spb - 1) / spb;
    const size_t in_sz = (size_t)NCW * rsdims, out_sz = (size_t)NMSG * rsdims;

    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t lsf = rsdims <= RS_THREADS ? tid / rsdims : 0u;  // local superframe of this lane
        const uint32_t lsfc = lsf < spb ? lsf : 0u;
        const long long sf = g * spb + lsf;
        if (tid < (int)spb) {
            s_sum[tid] = 0;
            s_fail[tid] = 0;
        }
        __syncthreads();
        for (uint32_t ch = 0; ch < nchunk; ch++) {
            if (tid < (int)spb) s_minfail[tid] = 0x7FFFFFFF;
            __syncthreads();
            const uint32_t colidx = rsdims <= RS_THREADS ? tid - lsf * rsdims : ch * RS_THREADS + tid;
            const bool active = lsf < spb && sf < nsf && colidx < rsdims && !s_fail[lsfc];
            if (active) {
                const uint8_t* src = p + (size_t)sf * in_sz + colidx;
                for (int k = 0; k < NCW; k++) cw[k * RS_THREADS + tid] = src[(size_t)k * rsdims];
            }
            const int res = decode_rs(active, lsf, cw, tid, ato, iof, mulp, qsol, step);  // all lanes
            if (res < 0) atomicMin(&s_minfail[lsf], (int)colidx);
            __syncthreads();
            const int mf = s_minfail[lsfc];
            if (active && (int)colidx < mf) {  // columns before the first failure are written
                uint8_t* dst = out + (size_t)sf * out_sz + colidx;
                for (int k = 0; k < NMSG; k++) dst[(size_t)k * rsdims] = cw[k * RS_THREADS + tid];
                atomicAdd(&s_sum[lsf], res);
            }
            __syncthreads();
            if (tid < (int)spb && s_minfail[tid] != 0x7FFFFFFF) s_fail[tid] = 1;
            __syncthreads();
        }
        if (tid < (int)spb && g * spb + tid < nsf) ret[g * spb + tid] = s_fail[tid] ? -1 : s_sum[tid];
        __syncthreads();
    }
}


// rsdims <= 256: spb = 256/rsdims superframes per pass, natural layout in LDS (see the header comment).
// LDS: 30720 (codewords) + 5120 (Chien steps) + 1024 (LFSR nibble rows) + 768 + 256 + 256 + 2048 = 40192 B: four workgroups
// share a CU (second launch bound: 4 waves per SIMD); a three-workgroup build was 6 % slower on clean data
// (profiles/r02_ab_rs_chien.txt).
__global__ __launch_bounds__(RS_THREADS, 4) void rs_kernel(const uint8_t* __restrict__ p, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ ret, uint32_t rsdims,
                                                        long long nsf, int host_polls_ret) {
    __shared__ __attribute__((aligned(16))) uint8_t cw[NCW * RS_THREADS];  // [superframe][row][column]
    __shared__ __attribute__((aligned(256))) uint32_t gnib[NIB_TABLES * 16 * 4];
    __shared__ uint32_t step[STEP_TERMS * 256];
    __shared__ uint8_t ato[ATO_SIZE];
    __shared__ uint8_t iof[256];
    __shared__ uint8_t qsol[256];
    __shared__ int s_minfail[RS_THREADS];
    __shared__ int s_sum[RS_THREADS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < ATO_SIZE; i += RS_THREADS) ato[i] = g_gf.ato[i];
    iof[tid] = g_gf.iof[tid];
    qsol[tid] = g_quad.q[tid];
    if (tid < (uint32_t)NIB_TABLES * 16u * 4u) gnib[tid] = g_nib.w[tid];
    for (uint32_t i = tid; i < STEP_TERMS * 256u; i += RS_THREADS) step[i] = g_step.w[i];
    __syncthreads();

    const uint32_t spb = RS_THREADS / rsdims;
    const long long ngroups = (nsf + spb - 1) / spb;
    const uint32_t in_sz = NCW * rsdims, out_sz = NMSG * rsdims;
    const uint32_t lsf = tid / rsdims, colidx = tid - lsf * rsdims;
    constexpr int NOFAIL = 0x7FFFFFFF;

    // The next group's input block is fetched into registers (8-byte words, 15 per thread) while the current
    // one is decoded, so the HBM latency of the load phase overlaps the LDS-bound decode of the same workgroup.
    constexpr uint32_t PRE = NCW * RS_THREADS / 8u / RS_THREADS;  // 15
    const bool pre_ok = (reinterpret_cast<uintptr_t>(p) & 7u) == 0;  // in_sz is a multiple of 8
    uint2 pre[PRE];
    auto prefetch = [&](long long gg) {
        const long long s0 = gg * spb;
        const uint32_t nl = nsf - s0 < (long long)spb ? (uint32_t)(nsf - s0) : spb;
        const uint32_t nw = nl * in_sz / 8u;
        const uint2* src = reinterpret_cast<const uint2*>(p + (size_t)s0 * in_sz);
#pragma unroll
        for (uint32_t k = 0; k < PRE; k++) {
            const uint32_t i = tid + k * RS_THREADS;
            pre[k] = i < nw ? src[i] : make_uint2(0u, 0u);
        }
    };
    if (pre_ok && (long long)blockIdx.x < ngroups) prefetch(blockIdx.x);

#ifndef RS_PRIO_ROT
#define RS_PRIO_ROT 1
#endif
#if RS_PRIO_ROT
    // Issue priority that rotates pass by pass (see vit_pk.hip: the hardware's arbitration otherwise lets the waves of a SIMD - here
    // one of each of the CU's four workgroups - advance one after the other): -3 % on clean data, -6 % with errors in 6 % of the columns
    // (profiles/r03_ab_rs_lfsr2.txt).  RS_PRIO_ROT = 2: the four waves of a workgroup share the level (the slot of wave 0).
    uint32_t rs_slot, rs_pass = 0;
    {
        uint32_t hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        rs_slot = hwid & 3u;
#if RS_PRIO_ROT == 2
        __shared__ uint32_t s_slot;
        if (tid == 0) s_slot = rs_slot;
        __syncthreads();
        rs_slot = s_slot;
        rs_slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs_slot);
#endif
    }
#endif
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
#if RS_PRIO_ROT
        if (ngroups > 2 * (long long)gridDim.x)  // a launch of one or two passes has nothing to level (and measured 2 % slower with it)
        switch ((rs_slot + rs_pass) & 3u) {
            case 0: __builtin_amdgcn_s_setprio(0); break;
            case 1: __builtin_amdgcn_s_setprio(1); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            default: __builtin_amdgcn_s_setprio(3); break;
        }
        rs_pass++;
#endif
        const long long sf0 = g * spb;
        const uint32_t nloc = nsf - sf0 < (long long)spb ? (uint32_t)(nsf - sf0) : spb;
        if (tid < spb) {
            s_minfail[tid] = NOFAIL;
            s_sum[tid] = 0;
        }
        if (pre_ok) {
            const uint32_t nw = nloc * in_sz / 8u;
#pragma unroll
            for (uint32_t k = 0; k < PRE; k++) {
                const uint32_t i = tid + k * RS_THREADS;
                if (i < nw) reinterpret_cast<uint2*>(cw)[i] = pre[k];
            }
            if (g + gridDim.x < ngroups) prefetch(g + gridDim.x);
        } else {
            copy_linear(cw, p + (size_t)sf0 * in_sz, nloc * in_sz, tid);
        }
        __syncthreads();
        const bool active = lsf < nloc;
        const int res = decode_rs_lfsr(active, lsf, cw, active ? lsf * in_sz + colidx : 0u, rsdims, ato, iof, qsol, gnib, step);  // all lanes
        if (res < 0) atomicMin(&s_minfail[lsf], (int)colidx);
        __syncthreads();
        uint8_t* dst0 = out + (size_t)sf0 * out_sz;
        // superframes without a failure: their first 110 rows go out as one linear block each
        if ((out_sz & 3u) == 0 && (reinterpret_cast<uintptr_t>(dst0) & 3u) == 0) {
            // 16-byte pieces when the block sizes and the destination allow it (in_sz is a multiple of 8, both are of 16
            // when rsdims is a multiple of 8), else dwords (the quotient c / wps in every trip of the plain loop was a
            // quarter of the clean path's instructions)
            if ((out_sz & 15u) == 0 && (in_sz & 15u) == 0 && (reinterpret_cast<uintptr_t>(dst0) & 15u) == 0)
                copy_out<uint4>(dst0, cw, s_minfail, nloc, in_sz, out_sz, tid);
            else
                copy_out<uint32_t>(dst0, cw, s_minfail, nloc, in_sz, out_sz, tid);
            if (active) {
                const int mf = s_minfail[lsf];
                if (mf != NOFAIL && (int)colidx < mf) {  // columns before the first failure are written
                    uint8_t* dst = dst0 + (lsf * out_sz + colidx);  // < 110 * 256
                    const uint8_t* src = cw + lsf * in_sz + colidx;
#pragma clang loop vectorize(disable) interleave(disable)
                    for (int k = 0; k < NMSG; k++) dst[(size_t)k * rsdims] = src[k * rsdims];
                }
                if ((int)colidx < mf) atomicAdd(&s_sum[lsf], res);
            }
        } else if (active) {
            const int mf = s_minfail[lsf];
            if ((int)colidx < mf) {
                uint8_t* dst = dst0 + (lsf * out_sz + colidx);  // < 110 * 256
                const uint8_t* src = cw + lsf * in_sz + colidx;
#pragma clang loop vectorize(disable) interleave(disable)
                for (int k = 0; k < NMSG; k++) dst[(size_t)k * rsdims] = src[k * rsdims];
                atomicAdd(&s_sum[lsf], res);
            }
        }
        // single-call path (RScheckSuperframe): the host spins on ret[0] in its mapped buffer instead of waiting for the
        // end-of-kernel signal, so every output byte must be visible system-wide before the return value is
        if (host_polls_ret) __threadfence_system();
        __syncthreads();
        if (tid < nloc) {
            const int32_t r = s_minfail[tid] != NOFAIL ? -1 : s_sum[tid];
            if (host_polls_ret) __hip_atomic_store(&ret[sf0 + tid], r, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            else ret[sf0 + tid] = r;
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t rs_launch(const uint8_t* d_p, uint8_t* d_out, int32_t* d_ret, uint32_t rsdims, int64_t nsf,
                     hipStream_t stream, bool host_polls_ret) {
    if (nsf <= 0 || rsdims == 0) return hipSuccess;
    if (host_polls_ret && (nsf != 1 || rsdims > RS_THREADS)) return hipErrorInvalidValue;
    const uint32_t spb = rsdims <= RS_THREADS ? RS_THREADS / rsdims : 1u;
    long long groups = (nsf + spb - 1) / spb;
    if (groups > (1 << 20)) groups = 1 << 20;
    if (rsdims <= RS_THREADS) {
        // persistent workgroups (4 fit a CU): each walks its groups with the next input block already in flight
        int dev = 0;
        const int cus = hipGetDevice(&dev) == hipSuccess ? vit_device_cus(dev) : 256;
        const long long resident = 4LL * cus;
        if (groups > resident) groups = resident;
    }
    if (rsdims <= RS_THREADS)
        hipLaunchKernelGGL(rs_kernel, dim3((unsigned)groups), dim3(RS_THREADS), 0, stream, d_p, d_out, d_ret, rsdims,
                           (long long)nsf, host_polls_ret ? 1 : 0);
    else
        hipLaunchKernelGGL(rs_kernel_wide, dim3((unsigned)groups), dim3(RS_THREADS), 0, stream, d_p, d_out, d_ret,
                           rsdims, (long long)nsf);
    return hipGetLastError();
}
