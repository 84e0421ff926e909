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
// What rs_kernel does with a pass - load, decode, first failure, copy-out, return values - is rs_dev.h's text, shared with
// rs_table_kernel (rs_table.hip); here is only the uniform arithmetic of a pass's place and the polled return's flag.
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


// rsdims <= 256: spb = 256/rsdims superframes per pass, natural layout in LDS (see the header comment); the pass itself is
// rs_dev.h's, shared with rs_table_kernel.
// LDS: 30720 (codewords) + 5120 (Chien steps) + 1024 (LFSR nibble rows) + 768 + 256 + 256 + 2048 = 40192 B: four workgroups
// share a CU (second launch bound: 4 waves per SIMD); a three-workgroup build was 6 % slower on clean data
// (profiles/r02_ab_rs_chien.txt).
constexpr bool RS_KERNEL_ROTATES_PRIO = true;  // rs_prio_rotate: measured here (round 3)
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
    rs_stage_tables(ato, iof, qsol, gnib, step, tid);
    __syncthreads();

    const uint32_t spb = RS_THREADS / rsdims;
    const long long ngroups = (nsf + spb - 1) / spb;
    const uint32_t in_sz = NCW * rsdims, out_sz = NMSG * rsdims;
    const uint32_t lsf = tid / rsdims, colidx = tid - lsf * rsdims;
    auto count = [&](long long gg) { return nsf - gg * spb < (long long)spb ? (uint32_t)(nsf - gg * spb) : spb; };  // superframes of group gg

    const bool pre_ok = (reinterpret_cast<uintptr_t>(p) & 7u) == 0;  // in_sz is a multiple of 8
    uint2 pre[RS_PRE];
    if (pre_ok && (long long)blockIdx.x < ngroups)
        rs_prefetch(pre, p + (size_t)blockIdx.x * spb * in_sz, count(blockIdx.x) * in_sz / 8u, tid);

    const uint32_t slot = RS_KERNEL_ROTATES_PRIO ? rs_prio_slot() : 0u;
    uint32_t pass = 0;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        if (RS_KERNEL_ROTATES_PRIO) rs_prio_rotate(slot, pass++, ngroups, gridDim.x);
        const long long sf0 = g * spb;
        const uint32_t nloc = count(g);
        rs_pass_reset(s_minfail, s_sum, spb, tid);
        const long long gn = g + gridDim.x;
        rs_pass_load(cw, pre, pre_ok, p, (size_t)sf0 * in_sz, nloc * in_sz, gn < ngroups, (size_t)gn * spb * in_sz,
                     count(gn) * in_sz, tid);
        __syncthreads();
        rs_pass_finish(cw, tid, rsdims, lsf, colidx, in_sz, out_sz, nloc, out + (size_t)sf0 * out_sz, ret + sf0,
                       host_polls_ret != 0, ato, iof, qsol, gnib, step, s_minfail, s_sum);
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
