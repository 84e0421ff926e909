// vit_internal.h -- launchers shared between the kernel TUs and the C-ABI TUs (whose own shared header is vit_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "viterbi_amd.h"

#define VIT_MAX_FRAMEBITS 9216u  // deconvolve.cpp:93,127 (384*24)
#define VIT_TAIL 6u              // K-1 tail steps
#define VIT_SORT_BINS (VIT_MAX_FRAMEBITS / 8u + 1u)  // counting-sort keys framebits/8

// renorm_ge (all decoder launchers): the renormalisation test on state 0.  false = `> 150`, the reference's C decoders
// (deconvolve.cpp:399,408; build configuration Rel_cpp); true = `>= 150`, its MASM decoders (decon_avx2.asm:97,114
// `cmp sil,150 ; jb mainloop`; Rel_asm, the configuration QIRX ships).  The two differ on hard-decision input from a
// poor channel, where path metrics reach the 0 / 255 clamps.
// Wave-per-frame kernel (lane = trellis state); any even framebits <= 9216.
hipError_t vit_launch_wave(const uint8_t* d_sym, uint8_t* d_out, const vit_frame_desc* d_desc,
                           uint32_t framebits, uint32_t max_framebits, int64_t nframes,
                           hipStream_t stream, bool renorm_ge);
// Packed kernel: 4 frames per wavefront, 2 states x 2 frames per lane register.
// Every even framebits <= 9216 (frames longer than 778 bits spill their history through HBM).
bool vit_pk_supported(uint32_t max_framebits);
// sym32: d_symbols holds the reference ABI's u32-per-symbol format (16-byte aligned; sym_offset
// then counts symbols); the narrowing to the low byte is fused into the kernel's pre-pass.
hipError_t vit_launch_pk(const void* d_symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                         uint32_t framebits, uint32_t max_framebits, int64_t nframes,
                         hipStream_t stream, bool renorm_ge);
// Packed kernel, 8 frames per wavefront at 2 wavefronts per SIMD (vit_pk8.hip): frames of one segment (framebits <= 778).
// An experiment, compiled in only with -DVIT_WITH_PK8 (otherwise vit_api_decode.hip holds stubs that report "not supported").
bool vit_pk8_supported(uint32_t max_framebits);
hipError_t vit_launch_pk8(const void* d_symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                          uint32_t framebits, uint32_t max_framebits, int64_t nframes, hipStream_t stream, bool renorm_ge);
// Latency kernel: one frame per wavefront, one path metric per lane, DPP partner fetches (small launches).
#define VIT_LAT_MAX_FRAMES 2048  // auto selection: up to two waves per SIMD; beyond that the packed kernel's throughput wins
// done_flag (optional, nframes == 1 only): a word in host-visible memory that receives done_seq, with system-scope
// release semantics, after the frame's last output byte.
hipError_t vit_launch_lat(const void* d_symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                          uint32_t framebits, uint32_t max_framebits, int64_t nframes,
                          hipStream_t stream, uint32_t* done_flag, uint32_t done_seq, bool renorm_ge);
// Ingest-stage launch (vit_ring.hip): one frame per slot of a mapped pinned ring.  The table travels BY VALUE in the
// kernel arguments (no descriptor fetch over PCIe in front of the symbol loads).
#define VIT_RING_MAXB 128u  // frames per launch
struct VitRingTable {
    uint32_t n;         // frames of this launch (= grid)
    uint32_t seq;       // what every slot's completion word receives (never 0)
    uint32_t stride;    // bytes per slot
    uint32_t out_off;   // offset of a slot's (framebits+7)/8 output bytes
    uint32_t flag_off;  // offset of a slot's completion word
    uint16_t slot[VIT_RING_MAXB];
    uint16_t fb[VIT_RING_MAXB];  // framebits of the frame in that slot (even, 2..9216)
};
hipError_t vit_launch_lat_ring(uint8_t* d_ring, const VitRingTable& tbl, uint32_t max_framebits, hipStream_t stream,
                               bool renorm_ge);
// frames the latency kernel can keep resident at one wave per SIMD or so for this frame length (LDS-limited)
int64_t vit_lat_capacity(uint32_t max_framebits, int dev);
// Length-sorted (longest first) copy of a device descriptor table; d_bins = 2*VIT_SORT_BINS words of scratch.
// bins_clean (optional): the caller's flag "the histogram half of d_bins is zero" - the scan kernel leaves it so; d_hdr (optional): 64
// words the scan kernel clears (the persistent kernel's counter header in front of the bins).
hipError_t vit_sort_descs_launch(const vit_frame_desc* d_desc, vit_frame_desc* d_sorted, int64_t nframes,
                                 uint32_t max_framebits, unsigned* d_bins, hipStream_t stream, bool* bins_clean = nullptr,
                                 unsigned* d_hdr = nullptr);
// Copy of a device descriptor table in which every descriptor that reaches outside [0, sym_bytes) / [0, out_bytes)
// has its framebits replaced by 0xFFFFFFFF (skipped by every kernel).
hipError_t vit_check_descs_launch(const vit_frame_desc* d_desc, vit_frame_desc* d_checked, int64_t nframes,
                                  uint64_t sym_bytes, uint64_t out_bytes, hipStream_t stream);
// u32 -> u8 narrowing (low byte), the reference ABI's symbol format to the device format.
hipError_t vit_launch_pack(const uint32_t* d_sym32, uint8_t* d_sym8, int64_t nsym,
                           hipStream_t stream);
// Depuncturing (vit_punct.hip).  Transmitted symbols of one frame under a HOST profile, or -1 (invalid profile, steps
// not summing to framebits + 6); start/base (optional, VIT_PUNCT_MAX_SEGS entries) receive each segment's first step
// and first transmitted byte.
int64_t vit_punct_length_host(const vit_punct_profile* p, uint32_t framebits, uint32_t* start, uint32_t* base);
// Uniform batch: frame f's transmitted bytes at d_punct + f*P, expanded into d_sym8 in the device format (frame f at
// f*4*(framebits+6)).  hipErrorInvalidValue for a profile that vit_punct_length_host rejects.
hipError_t vit_launch_depunct(const uint8_t* d_punct, uint8_t* d_sym8, uint32_t framebits, int64_t nframes,
                              const vit_punct_profile* profile, uint8_t erasure, hipStream_t stream);
// Variable-length batch with per-frame DEVICE profiles (desc[i].reserved = profile index): frame i is expanded into
// d_slots + i*4*(max_framebits+6) and d_idesc[i] receives its internal descriptor - framebits 0xFFFFFFFF (skipped by
// every decoder) for a descriptor that fails a check of vit_decode_punctured_varlen_dev.
hipError_t vit_launch_depunct_varlen(const uint8_t* d_punct, uint64_t sym_bytes, uint64_t out_bytes, const vit_frame_desc* d_desc,
                                     int64_t nframes, uint32_t max_framebits, const vit_punct_profile* d_profiles,
                                     uint32_t nprofiles, uint8_t erasure, uint8_t* d_slots, vit_frame_desc* d_idesc,
                                     hipStream_t stream);
// MSC time de-interleaving (vit_ti.hip); the caller has checked the ring (include/viterbi_amd.h, vit_cif_ring: the
// call's nframes + 15 rows distinct, its columns inside row_bytes).  Standalone: frame n's ncols bytes to d_out + n*ncols.
hipError_t vit_launch_time_deinterleave(const vit_cif_ring& ring, uint64_t col, uint32_t ncols, uint8_t* d_out,
                                        int64_t nframes, hipStream_t stream);
// Fused with the expansion: as vit_launch_depunct, frame n's transmitted symbols read from the ring at columns
// [col, col + P).
hipError_t vit_launch_depunct_ti(const vit_cif_ring& ring, uint64_t col, uint8_t* d_sym8, uint32_t framebits, int64_t nframes,
                                 const vit_punct_profile* profile, uint8_t erasure, hipStream_t stream);
// From the FFT (vit_ofdm.hip).  The standard's frequency interleaving as FFT bins (include/viterbi_amd.h,
// vit_freq_interleave_bins): K = 3*nfft/4 bins to h_bins, or -1.
int64_t vit_freq_bins_host(uint32_t nfft, uint16_t* h_bins);
// Demaps nframes transmission frames; the caller has checked every argument rule of vit_ofdm_demap_dev.  d_fic / ring may
// be NULL (those symbols are skipped).  rule: VIT_SOFT_PER_CARRIER (the existing kernels; d_level NULL) or
// VIT_SOFT_PER_SYMBOL (the kernels of the per-symbol rule; d_level NULL or nframes * (nsyms-1) floats).
hipError_t vit_launch_ofdm_demap(const float* d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t* d_bins,
                                 const vit_ofdm_shape& shape, float gain, int64_t nframes, uint8_t* d_fic,
                                 const vit_cif_ring* ring, uint64_t col, uint32_t rule, float* d_level, hipStream_t stream);
// From the samples (vit_ofdm_td.hip).  The tables of include/viterbi_amd.h: pairs written, or -1.
int64_t vit_fft_twiddles_host(uint32_t nfft, float* h_tw);
int64_t vit_nco_table_host(uint32_t nco_bits, float* h_nco);
// Rotation and FFT of nframes frames, then the spectra to d_fft (vit_launch_ofdm_fft) or the demapping of
// vit_launch_ofdm_demap without a spectrum in memory (vit_launch_ofdm_demod); the caller has checked every argument rule.
// fmt: the samples' format (format and scale checked by the caller; VIT_IQ_F32 ignores the scale).
hipError_t vit_launch_ofdm_fft(const vit_iq_input& in, const vit_iq_format& fmt, uint32_t nfft, uint32_t nsyms, int64_t nframes, float* d_fft,
                               uint64_t out_sym_stride, uint64_t out_frame_stride, hipStream_t stream);
hipError_t vit_launch_ofdm_demod(const vit_iq_input& in, const vit_iq_format& fmt, const uint16_t* d_bins, const vit_ofdm_shape& shape, float gain,
                                 int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring, uint64_t col, uint32_t rule, float* d_level,
                                 hipStream_t stream);
// From the coarse start (vit_ofdm_sync.hip): one workgroup per frame; the caller has checked every argument rule.
hipError_t vit_launch_ofdm_sync(const vit_iq_input& in, const vit_iq_format& fmt, const vit_sync_params& p, const float* d_prs, int64_t nframes,
                                int64_t* d_start_out, uint32_t* d_rot_out, uint32_t* d_info, hipStream_t stream);
// From the stream (vit_ofdm_acq.hip); the caller has checked every argument rule.  The power of blocks 0 ... nblk-1 of B
// samples behind sample `first` to d_power, then the search of nperiods periods on them (nblk: the blocks the stream
// holds, which decide the candidates that exist - the search reads powers 0 ... min(nblk, Ln + nperiods*Pb + Lr - 1) - 1).
hipError_t vit_launch_acq_power(const void* d_iq, const vit_iq_format& fmt, uint64_t first, uint32_t B, uint64_t nblk, float* d_power,
                                hipStream_t stream);
hipError_t vit_launch_acq_search(const float* d_power, uint64_t nblk, const vit_acq_params& p, int64_t nperiods, int64_t* d_start_out,
                                 uint32_t* d_info, hipStream_t stream);
// Before the stream (vit_resample.hip); the caller has checked every argument rule, nout <= vit_resample_out_count among
// them.  fmt as above; p.rot is read during the call (it travels in the kernel arguments).
hipError_t vit_launch_resample(const void* d_iq, const vit_iq_format& fmt, const vit_resample_params& p, int64_t nout, float* d_out,
                               uint64_t out_stride, hipStream_t stream);
// Transmitter identification (vit_ofdm_tii.hip); the caller has checked every argument rule.  One workgroup per frame
// writes the frame's Gp*C pair powers to row t of d_slots (nframes rows; a skipped frame's row is neither written nor
// read), then one workgroup per group of navg frames writes the group's words of d_tii and, if given, of d_energy.
hipError_t vit_launch_ofdm_tii(const vit_iq_input& in, const vit_iq_format& fmt, const vit_tii_params& p, const uint16_t* d_pairs,
                               int64_t nframes, float* d_slots, uint32_t* d_tii, float* d_energy, hipStream_t stream);
// Integer samples to the floats of the definition (vit_iq_convert.hip): 2*nsamples floats to d_out; fmt is an integer
// format, checked by the caller like the alignments.
hipError_t vit_launch_iq_convert(const void* d_iq, const vit_iq_format& fmt, uint64_t nsamples, float* d_out, hipStream_t stream);
// After the decoder (vit_dab.hip).  The energy dispersal PRBS of one frame, (framebits+7)/8 bytes, padding bits 0
// (framebits even, <= 9216; the caller checks).
int64_t vit_prbs_bytes_host(uint8_t* h_out, uint32_t framebits);
// In place: nframes frames of (framebits+7)/8 bytes back to back XORed with the PRBS.
hipError_t vit_launch_disperse(uint8_t* d_bytes, uint32_t framebits, int64_t nframes, hipStream_t stream);
// In place over a descriptor table (out_offset, framebits); descriptors with odd framebits, framebits > 9216 or output
// bytes outside [0, out_bytes) are skipped.
hipError_t vit_launch_disperse_varlen(uint8_t* d_bytes, uint64_t out_bytes, const vit_frame_desc* d_desc, int64_t nframes,
                                      hipStream_t stream);
// nfibs 32-byte FIBs back to back, fibs_per_frame of them per frame: descrambled in place first if `descramble`
// (d_fibs is only read otherwise), then d_ok[i] = 1 if FIB i's CRC-16 holds, else 0.
hipError_t vit_launch_fibs(uint8_t* d_fibs, int64_t nfibs, uint32_t fibs_per_frame, bool descramble, uint8_t* d_ok,
                           hipStream_t stream);
// DAB+: 5*nsf frames of 24*rsdims bytes descrambled in place; d_fire_ok[s] (optional) = the fire code of superframe s
// on its descrambled bytes 0..10.
hipError_t vit_launch_dabplus_post(uint8_t* d_work, uint32_t rsdims, int64_t nsf, uint8_t* d_fire_ok, hipStream_t stream);
// DAB+ access units: one vit_au_table per superframe of 110*rsdims bytes at d_sf + s*sf_stride (d_ret optional: a
// negative value gives VIT_AU_RS_FAILED without reading the superframe); the host form takes one superframe.
hipError_t vit_launch_aus(const uint8_t* d_sf, uint64_t sf_stride, uint32_t rsdims, int64_t nsf, const int32_t* d_ret,
                          vit_au_table* d_au, hipStream_t stream);
void vit_au_table_host(const uint8_t* h_sf, uint32_t rsdims, vit_au_table* h_out);
// d_ok[i] = the fire code of the 11 bytes at d_bytes + i*stride.
hipError_t vit_launch_fire(const uint8_t* d_bytes, uint64_t stride, int64_t n, uint8_t* d_ok, hipStream_t stream);
// Packet mode (vit_packet.hip); the caller has checked every argument rule.  vit_launch_fec_sync clears d_score (a memset
// on the stream) in front of its kernel; vit_launch_fec with d_out != d_stream launches even without a whole frame, for
// the copy; the host form takes one FEC frame of 2472 bytes.
hipError_t vit_launch_fec_sync(const uint8_t* d_stream, int64_t nslots, uint32_t* d_score, hipStream_t stream);
hipError_t vit_launch_fec(const uint8_t* d_stream, uint8_t* d_out, int64_t nslots, uint32_t phase, int64_t nfec, vit_fec_rec* d_fec,
                          hipStream_t stream);
void vit_fec_frame_host(uint8_t* frame, vit_fec_rec* h_out);
hipError_t vit_launch_packets(const uint8_t* d_bytes, uint32_t framebytes, int64_t nframes, vit_packet_rec* d_rec,
                              hipStream_t stream);
// Packet mode for a table of streams (vit_packet_table.hip; include/viterbi_amd.h, vit_pkt_stream): the table as the
// kernels read it, BY VALUE in the kernel arguments.  Entry k holds where stream k's bytes and records start and where
// its share of each stage's passes starts; a pass finds its stream with vit_table_find - an entry without passes in a
// stage (a stream that is not FEC_SEARCH among the sync workgroups) is never the answer.  The ranges end at the totals.
struct VitPktEntry {
    uint64_t offset;    // bytes from d_bytes
    uint32_t nframes;   // logical frames
    uint32_t nslots;    // nframes * S
    uint32_t rec0;      // first vit_packet_rec (slots of earlier streams)
    uint32_t fec0;      // first vit_fec_rec
    uint32_t pkt0;      // first packet pass: a wavefront's round of 64 / S logical frames of ONE stream
    uint32_t sync0;     // first sync workgroup: one per VIT_PKT_SYNC_CHUNK slots of a FEC_SEARCH stream
    uint32_t fecwg0;    // first FEC workgroup: one per 20 FEC frames the stream can hold at most (at its given phase)
    uint8_t S;          // slots per logical frame, 1 ... 48
    uint8_t fec;        // VIT_PKT_FEC_*
    uint8_t phase;      // FEC_PHASE: the host's phase
    uint8_t pad;
};
#define VIT_PKT_SYNC_CHUNK 1024u  // slots: four per thread, as the uniform launch's grid
struct VitPktTable {
    uint32_t nstreams, npkt, nsync, nfecwg;  // the totals
    VitPktEntry e[VIT_PKT_MAX_STREAMS];
};
static_assert(sizeof(VitPktEntry) == 40 && sizeof(VitPktTable) == 16 + 40 * VIT_PKT_MAX_STREAMS && sizeof(VitPktTable) + 64 <= 4096,
              "2576 bytes: the table and five pointers fit the 4 KB of kernel arguments");
// The launches of vit_packet_table_dev, in order; the caller has checked every argument rule.  d_score: 103 words per
// stream, cleared on the stream in front of the sync kernel (vit_launch_pkt_table_sync does both; it is called only when
// the scores are wanted - a FEC_SEARCH entry, or the caller's d_score); the pick reads them only for FEC_SEARCH entries
// and writes every stream's vit_pkt_stream_rec; the FEC workgroups read phase and nfec from d_srec.
hipError_t vit_launch_pkt_table_sync(const uint8_t* d_bytes, const VitPktTable& tab, uint32_t* d_score, hipStream_t stream);
hipError_t vit_launch_pkt_table_pick(const VitPktTable& tab, const uint32_t* d_score, const uint32_t* h_min_score,
                                     vit_pkt_stream_rec* d_srec, hipStream_t stream);
hipError_t vit_launch_pkt_table_fec(uint8_t* d_bytes, const VitPktTable& tab, const vit_pkt_stream_rec* d_srec, vit_fec_rec* d_fec,
                                    hipStream_t stream);
hipError_t vit_launch_pkt_table_packets(const uint8_t* d_bytes, const VitPktTable& tab, vit_packet_rec* d_rec, hipStream_t stream);
// Data groups (vit_dgroup.hip); the caller has checked every argument rule.  d_scratch: vit_data_groups_scratch(nslots)
// bytes, 16-byte aligned; its first 256 bytes are cleared on the stream in front of the kernels.  The host form is the
// same definition as a walk per address.
size_t vit_data_groups_scratch(int64_t nslots);
hipError_t vit_launch_data_groups(const uint8_t* d_bytes, const vit_packet_rec* d_rec, int64_t nslots, vit_dgroup_rec* d_dg,
                                  uint32_t max_groups, vit_dgroup_summary* d_sum, uint8_t* d_data, uint32_t data_capacity,
                                  void* d_scratch, hipStream_t stream);
void vit_data_groups_host_impl(const uint8_t* bytes, const vit_packet_rec* rec, int64_t nslots, vit_dgroup_rec* dg, uint32_t max_groups,
                               vit_dgroup_summary* sum, uint8_t* data, uint32_t data_capacity);
// Multiplex configuration (vit_mci.hip); the caller has checked every argument rule.  One launch; the host form is the
// same walk on host memory.
hipError_t vit_launch_mci(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* d_sub,
                          vit_mci_group* d_grp, uint8_t* d_status, hipStream_t stream);
void vit_mci_fibs_host_impl(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* h_sub,
                            vit_mci_group* h_grp, uint8_t* h_status);
// Service directory (vit_mci_dir.hip); the caller has checked every argument rule.  One launch; the host form is the same
// walk on host memory.
hipError_t vit_launch_mci_dir(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* d_svc,
                              vit_mci_pktcomp* d_pkt, vit_mci_dir* d_dir, uint8_t* d_status, hipStream_t stream);
void vit_mci_dir_host_impl(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* h_svc,
                           vit_mci_pktcomp* h_pkt, vit_mci_dir* h_dir, uint8_t* h_status);
// RS(120,110) superframe check, one lane per column.
// host_polls_ret (nsf == 1, rsdims <= 256): d_ret is host-visible and receives its value with system-scope release
// semantics after the last output byte, so the host may spin on it instead of synchronising the stream.
hipError_t rs_launch(const uint8_t* d_p, uint8_t* d_out, int32_t* d_ret, uint32_t rsdims,
                     int64_t nsf, hipStream_t stream, bool host_polls_ret = false);
// A whole ensemble (include/viterbi_amd.h, vit_ens_subch): the sub-channel table as the kernels read it, BY VALUE in the
// kernel arguments (2 KB).  Entry k holds where sub-channel k's blocks and its index ranges start; every kernel finds the
// sub-channel of an index x (a frame, a record, an RS pass) as the largest k whose start is <= x - an entry with an
// empty range, such as one that is not DAB+ among the records, is never the answer.  The ranges end at the totals.
struct VitEnsEntry {
    uint64_t work_off, rs_off;  // vit_ens_layout's
    uint32_t rec0;              // first record (superframe)
    uint32_t frame0;            // first frame, all sub-channels counted
    uint32_t pass0;             // first RS pass: a workgroup pass takes 256 / rsdims superframes of ONE sub-channel
    uint16_t framebits, rsdims;
};
struct VitEnsTable {
    uint32_t nsub, nframes, nrec, npass;  // the totals
    uint32_t max_rsdims, pad[3];
    VitEnsEntry e[VIT_ENS_MAX_SUBCH];
};
// The lookup of every table that travels in the kernel arguments (VitEnsTable and VitPktTable above, VitDgTable below):
// vit_table_find<Entry, &Entry::start>(e, n, x) is the largest k < n with e[k].start <= x, for starts that do not
// decrease and begin with e[0].start == 0.
template <class Entry, uint32_t Entry::*START>
__host__ __device__ inline uint32_t vit_table_find(const Entry* e, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;  // e[0]'s start is 0
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (e[mid].*START <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Data groups for a table of streams (vit_dgroup_table.hip; include/viterbi_amd.h, vit_dg_stream): the table as the kernels
// read it, BY VALUE in the kernel arguments.  Entry k holds where stream k's bytes, records and outputs start, where its
// scratch arrays start and where its share of each stage's workgroups starts; a workgroup finds its stream with
// vit_table_find.  Every stream has at least one slot, so it owns at least one workgroup of every stage but the link
// totals, whose share is derived: a stream of nchunks chunks owns nchunks - 1 of them, from chunk0 - k on.  The gather
// numbers the groups that are written over the table on the device, from the streams' headers.  What else the kernels
// need of a stream - the places of its scratch arrays behind scr0, its chunks and blocks - follows from nslots.
struct VitDgEntry {
    uint64_t offset;      // bytes from d_bytes
    uint64_t rec0;        // first vit_packet_rec
    uint32_t nslots;
    uint32_t max_groups;
    uint32_t capacity;
    uint32_t has_data;    // 0: records only, as with d_data NULL
    uint32_t dg0;         // first vit_dgroup_rec (vit_dg_layout.dg_index)
    uint32_t data0;       // its block of d_data (vit_dg_layout.data_offset)
    uint32_t scr0;        // its scratch arrays behind the table's headers, in units of 16 bytes from the scratch's start
    uint32_t chunk0;      // first link workgroup column: one per 16384 slots (and per address)
    uint32_t blk0;        // first presence, sums and place workgroup: one per 4096 slots
    uint32_t pad;         // 0
};
struct VitDgTable {
    uint32_t nstreams, nchunk, nblk;  // the totals
    uint32_t ngat;                    // gather passes: max(1, min(max_groups, nslots)) per stream, the most groups it can write
    VitDgEntry e[VIT_DG_MAX_STREAMS];
};
static_assert(sizeof(VitDgEntry) == 56 && sizeof(VitDgTable) == 16 + 56 * VIT_DG_MAX_STREAMS && sizeof(VitDgTable) + 64 <= 4096,
              "3600 bytes: the table and the gather's six pointers fit the 4 KB of kernel arguments");
// Fills scr0, chunk0, blk0 and the totals from the entries' nslots and max_groups; returns the scratch the launches
// need: the streams' 256-byte headers back to back, then every stream's arrays.
size_t vit_dg_table_geometry(VitDgTable* tab);
// The launches of vit_data_groups_table_dev; the caller has checked every argument rule.  d_scratch: what
// vit_dg_table_geometry returned, 16-byte aligned; the headers are cleared on the stream in front of the kernels.
hipError_t vit_launch_data_groups_table(const uint8_t* d_bytes, const vit_packet_rec* d_rec, const VitDgTable& tab, vit_dgroup_rec* d_dg,
                                        vit_dgroup_summary* d_sum, uint8_t* d_data, void* d_scratch, hipStream_t stream);
// vit_ens_find<&VitEnsEntry::frame0>(tab, x): the sub-channel whose frames hold frame x < tab.nframes (rec0, pass0 alike)
template <uint32_t VitEnsEntry::*START>
__host__ __device__ inline uint32_t vit_ens_find(const VitEnsTable& tab, uint32_t x) {
    return vit_table_find<VitEnsEntry, START>(tab.e, tab.nsub, x);
}
// what only the descriptor kernel needs of a sub-channel
struct VitEnsSource {
    uint32_t sym0[VIT_ENS_MAX_SUBCH];  // its first column within the de-interleaved span
    uint32_t phase[VIT_ENS_MAX_SUBCH], profile[VIT_ENS_MAX_SUBCH];
};
// The chain's launches, in order (vit_ensemble_dev; the caller has checked every argument rule):
//   vit_launch_time_deinterleave   the span of columns the table uses, frames 0 ... max(phase + nframes) - 1
//   vit_launch_ens_descs           d_desc[i] for frame i of the table: its symbols in the de-interleaved copy (frame
//                                  phase + j of the span, `span` bytes per frame), its bytes in d_work, its profile
//   vit_launch_depunct_varlen      expansion into the slots, checked descriptors to a second table
//   launch_decode                  (vit_host.h)
//   vit_launch_ens_post            every frame descrambled in place, the fire code of every DAB+ superframe's first
//                                  frame to d_fire_ok (optional); a frame whose checked descriptor (d_idesc, optional) is
//                                  marked as skipped is not descrambled
//   rs_table_launch                RS over every DAB+ sub-channel
//   vit_launch_aus_table           access units; from_work: superframes read from the work layout (120*rsdims apart)
hipError_t vit_launch_ens_descs(const VitEnsTable& tab, const VitEnsSource& src, uint64_t span, vit_frame_desc* d_desc,
                                hipStream_t stream);
hipError_t vit_launch_ens_post(uint8_t* d_work, const VitEnsTable& tab, const vit_frame_desc* d_idesc, uint8_t* d_fire_ok,
                               hipStream_t stream);
hipError_t rs_table_launch(const uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret, const VitEnsTable& tab, hipStream_t stream);
hipError_t vit_launch_aus_table(const uint8_t* d_sf, bool from_work, const VitEnsTable& tab, const int32_t* d_ret,
                                vit_au_table* d_au, hipStream_t stream);

// ---- host-side helpers shared by the TUs -------------------------------------------------------
// per-thread error text behind vit_last_error() (printf-style)
void vit_set_err(const char* fmt, ...);
// CU count of a HIP device, cached (persistent grids are sized by it)
int vit_device_cus(int dev);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: opt the kernels in once per (device, caller).
// `done` is the caller's bitmask of devices already handled (guarded by an internal mutex).
hipError_t vit_optin_dynamic_lds(const void* const* kernels, int nkernels, int bytes, int dev, uint64_t* done);
// Launches KERNEL with `lds` bytes of dynamic LDS; where that is more than the 64 KiB a kernel gets by default, KERNEL is
// first opted in on the current device.  KERNEL is a template argument, so every kernel has a `done` mask of its own.
template <auto KERNEL, typename... Args>
hipError_t vit_launch_dynamic_lds(unsigned grid, unsigned block, size_t lds, hipStream_t stream, const Args&... args) {
    if (lds > 64u * 1024u) {
        static uint64_t optin_done = 0;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        const void* ks[1] = {reinterpret_cast<const void*>(KERNEL)};
        const hipError_t e = vit_optin_dynamic_lds(ks, 1, 160 * 1024, dev, &optin_done);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), lds, stream, args...);
    return hipGetLastError();
}
// Restores the calling thread's current HIP device on scope exit (library calls must not leave it changed).
struct VitDeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit VitDeviceGuard(int want) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (want >= 0 && prev != want && hipSetDevice(want) == hipSuccess) changed = true;
    }
    ~VitDeviceGuard() {
        if (changed && prev >= 0) (void)hipSetDevice(prev);
    }
    VitDeviceGuard(const VitDeviceGuard&) = delete;
    VitDeviceGuard& operator=(const VitDeviceGuard&) = delete;
};
