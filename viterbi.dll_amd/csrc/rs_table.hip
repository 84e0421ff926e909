// rs_table.hip -- RS(120,110) over a table of sub-channels of different widths in one launch (include/viterbi_amd.h,
// vit_rs_table_dev): rs_kernel of rs_kernels.hip with the pass's width, place and count taken from the table.  The pass
// itself is rs_dev.h's one text; this unit holds the table lookup, one pass ahead.
#include "rs_dev.h"

namespace {

// rs_kernel over a table of sub-channels (vit_internal.h, VitEnsTable): pass g of the launch belongs to the sub-channel
// whose range of passes holds it and takes 256 / rsdims of ITS superframes, so a pass never mixes sub-channels and
// everything below the pass (decode_rs_lfsr, the first-failure rule per superframe) is the shared text.  The register
// prefetch of the workgroup's next pass goes on across a sub-channel boundary: the next pass's place is looked up one
// pass ahead.  The table's offsets are multiples of 16, so the 8-byte prefetch depends on the alignment of p alone.
struct RsPass {
    uint32_t rsdims, sf0, nloc;  // the pass's sub-channel width, first superframe within the sub-channel, superframes
    uint64_t in_off, out_off;    // of superframe sf0: bytes from p / out
    uint32_t rec;                // and its record
};
__device__ __forceinline__ RsPass rs_table_pass(const VitEnsTable& tab, uint32_t g) {
    const uint32_t k = vit_ens_find<&VitEnsEntry::pass0>(tab, g);
    const VitEnsEntry& e = tab.e[k];
    const uint32_t nsf = (k + 1u < tab.nsub ? tab.e[k + 1u].rec0 : tab.nrec) - e.rec0;
    RsPass ps;
    ps.rsdims = e.rsdims;
    const uint32_t spb = RS_THREADS / ps.rsdims;
    ps.sf0 = (g - e.pass0) * spb;
    ps.nloc = nsf - ps.sf0 < spb ? nsf - ps.sf0 : spb;
    ps.in_off = e.work_off + (uint64_t)ps.sf0 * (NCW * ps.rsdims);
    ps.out_off = e.rs_off + (uint64_t)ps.sf0 * (NMSG * ps.rsdims);
    ps.rec = e.rec0 + ps.sf0;
    return ps;
}

// rs_prio_rotate is NOT used here, and never was: the build switch that guarded it in this unit was given its value in
// rs_kernels.hip alone, so the rotation was never compiled into this kernel, and the round-18 figures
// (profiles/r18_ensemble_bench.json) are for the kernel without it.  Turning it on is a performance change that nobody
// has measured, not a correction.
constexpr bool RS_TABLE_ROTATES_PRIO = false;
__global__ __launch_bounds__(RS_THREADS, 4) void rs_table_kernel(const uint8_t* __restrict__ p, uint8_t* __restrict__ out,
                                                                 int32_t* __restrict__ ret, const VitEnsTable tab) {
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

    const bool pre_ok = (reinterpret_cast<uintptr_t>(p) & 7u) == 0;
    const uint32_t npass = tab.npass;
    uint2 pre[RS_PRE];
    RsPass next = {};
    if (blockIdx.x < npass) {
        next = rs_table_pass(tab, blockIdx.x);
        if (pre_ok) rs_prefetch(pre, p + next.in_off, next.nloc * (NCW * next.rsdims) / 8u, tid);  // <= 15 * 256 words
    }
    const uint32_t slot = RS_TABLE_ROTATES_PRIO ? rs_prio_slot() : 0u;
    uint32_t pass = 0;
    for (uint32_t g = blockIdx.x; g < npass; g += gridDim.x) {
        if (RS_TABLE_ROTATES_PRIO) rs_prio_rotate(slot, pass++, npass, gridDim.x);
        const RsPass ps = next;
        const uint32_t rsdims = ps.rsdims, in_sz = NCW * rsdims, out_sz = NMSG * rsdims;
        const uint32_t lsf = tid / rsdims, colidx = tid - lsf * rsdims;
        rs_pass_reset(s_minfail, s_sum, RS_THREADS / rsdims, tid);
        const bool more = g + gridDim.x < npass;  // (npass <= 2^31: no wrap)
        if (more) next = rs_table_pass(tab, g + gridDim.x);
        rs_pass_load(cw, pre, pre_ok, p, ps.in_off, ps.nloc * in_sz, more, next.in_off, next.nloc * (NCW * next.rsdims), tid);
        __syncthreads();
        rs_pass_finish(cw, tid, rsdims, lsf, colidx, in_sz, out_sz, ps.nloc, out + ps.out_off, ret + ps.rec, false, ato, iof,
                       qsol, gnib, step, s_minfail, s_sum);
        __syncthreads();
    }
}

}  // namespace

hipError_t rs_table_launch(const uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret, const VitEnsTable& tab, hipStream_t stream) {
    if (tab.npass == 0) return hipSuccess;
    int dev = 0;
    const unsigned resident = 4u * (unsigned)(hipGetDevice(&dev) == hipSuccess ? vit_device_cus(dev) : 256);
    hipLaunchKernelGGL(rs_table_kernel, dim3(tab.npass < resident ? tab.npass : resident), dim3(RS_THREADS), 0, stream, d_work,
                       d_rs_out, d_ret, tab);
    return hipGetLastError();
}
