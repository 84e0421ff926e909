// rs_table.hip -- RS(120,110) over a table of sub-channels of different widths in one launch (include/viterbi_amd.h,
// vit_rs_table_dev): rs_kernel of rs_kernels.hip with the pass's width, place and count taken from the table.
#include "rs_dev.h"

namespace {

// A pass behind its load, the second half of rs_kernel's loop body (that kernel keeps its own text of it, so that its code
// is what it was), without the single-call export's polled return value: cw holds nloc superframes of rsdims columns in their natural layout (in_sz bytes each), s_minfail /
// s_sum are reset and the barrier behind all that is passed.  Decodes, writes the superframes' out_sz output bytes from
// dst0 on and their return values from ret0 on.  lsf / colidx: this lane's superframe of the pass and column in it.  Ends
// in front of the pass's last barrier.
__device__ __forceinline__ void rs_pass_finish(uint8_t* cw, uint32_t tid, uint32_t rsdims, uint32_t lsf, uint32_t colidx,
                                               uint32_t in_sz, uint32_t out_sz, uint32_t nloc, uint8_t* dst0, int32_t* ret0,
                                               const uint8_t* ato, const uint8_t* iof, const uint8_t* qsol, const uint32_t* gnib,
                                               const uint32_t* step, int* s_minfail, int* s_sum) {
    constexpr int NOFAIL = 0x7FFFFFFF;
    const bool active = lsf < nloc;
    const int res = decode_rs_lfsr(active, lsf, cw, active ? lsf * in_sz + colidx : 0u, rsdims, ato, iof, qsol, gnib, step);  // all lanes
    if (res < 0) atomicMin(&s_minfail[lsf], (int)colidx);
    __syncthreads();
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
    __syncthreads();
    if (tid < nloc) ret0[tid] = s_minfail[tid] != NOFAIL ? -1 : s_sum[tid];
}

// rs_kernel over a table of sub-channels (vit_internal.h, VitEnsTable): pass g of the launch belongs to the sub-channel
// whose range of passes holds it and takes 256 / rsdims of ITS superframes, so a pass never mixes sub-channels and
// everything below the pass (decode_rs_lfsr, the first-failure rule per superframe) is rs_kernel's.  The register
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
    for (uint32_t i = tid; i < ATO_SIZE; i += RS_THREADS) ato[i] = g_gf.ato[i];
    iof[tid] = g_gf.iof[tid];
    qsol[tid] = g_quad.q[tid];
    if (tid < (uint32_t)NIB_TABLES * 16u * 4u) gnib[tid] = g_nib.w[tid];
    for (uint32_t i = tid; i < STEP_TERMS * 256u; i += RS_THREADS) step[i] = g_step.w[i];
    __syncthreads();

    constexpr int NOFAIL = 0x7FFFFFFF;
    constexpr uint32_t PRE = NCW * RS_THREADS / 8u / RS_THREADS;  // 15
    const bool pre_ok = (reinterpret_cast<uintptr_t>(p) & 7u) == 0;
    const uint32_t npass = tab.npass;
    uint2 pre[PRE];
    auto prefetch = [&](const RsPass& ps) {
        const uint32_t nw = ps.nloc * (NCW * ps.rsdims) / 8u;  // <= 15 * 256
        const uint2* src = reinterpret_cast<const uint2*>(p + ps.in_off);
#pragma unroll
        for (uint32_t k = 0; k < PRE; k++) {
            const uint32_t i = tid + k * RS_THREADS;
            pre[k] = i < nw ? src[i] : make_uint2(0u, 0u);
        }
    };
    RsPass next = {};
    if (blockIdx.x < npass) {
        next = rs_table_pass(tab, blockIdx.x);
        if (pre_ok) prefetch(next);
    }
#if RS_PRIO_ROT
    uint32_t rs_slot, rs_pass = 0;  // as rs_kernel
    {
        uint32_t hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        rs_slot = hwid & 3u;
    }
#endif
    for (uint32_t g = blockIdx.x; g < npass; g += gridDim.x) {
#if RS_PRIO_ROT
        if (npass > 2u * gridDim.x)
        switch ((rs_slot + rs_pass) & 3u) {
            case 0: __builtin_amdgcn_s_setprio(0); break;
            case 1: __builtin_amdgcn_s_setprio(1); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            default: __builtin_amdgcn_s_setprio(3); break;
        }
        rs_pass++;
#endif
        const RsPass ps = next;
        const uint32_t rsdims = ps.rsdims, in_sz = NCW * rsdims, out_sz = NMSG * rsdims;
        const uint32_t lsf = tid / rsdims, colidx = tid - lsf * rsdims;
        if (tid < RS_THREADS / rsdims) {
            s_minfail[tid] = NOFAIL;
            s_sum[tid] = 0;
        }
        const bool more = g + gridDim.x < npass;  // (npass <= 2^31: no wrap)
        if (more) next = rs_table_pass(tab, g + gridDim.x);
        if (pre_ok) {
            const uint32_t nw = ps.nloc * in_sz / 8u;
#pragma unroll
            for (uint32_t k = 0; k < PRE; k++) {
                const uint32_t i = tid + k * RS_THREADS;
                if (i < nw) reinterpret_cast<uint2*>(cw)[i] = pre[k];
            }
            if (more) prefetch(next);
        } else {
            copy_linear(cw, p + ps.in_off, ps.nloc * in_sz, tid);
        }
        __syncthreads();
        rs_pass_finish(cw, tid, rsdims, lsf, colidx, in_sz, out_sz, ps.nloc, out + ps.out_off, ret + ps.rec, ato, iof, qsol, gnib,
                       step, s_minfail, s_sum);
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
