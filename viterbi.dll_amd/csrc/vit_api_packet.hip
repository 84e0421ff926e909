// vit_api_packet.hip -- the C ABI of packet mode (include/viterbi_amd.h, "Packet mode"): argument rules and launches
// only; the kernels and the host twin are in vit_packet.hip, the format's constants in vit_packet_fmt.h.
#include "vit_host.h"
#include "vit_packet_fmt.h"

using namespace pktfmt;

namespace {

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
// whole FEC frames in nslots slots from `phase` on (nslots >= 0, phase < 103)
inline int64_t fec_count(int64_t nslots, uint32_t phase) { return nslots > (int64_t)phase ? (nslots - phase) / FEC_SLOTS : 0; }

}  // namespace

int64_t vit_packet_fec_count(int64_t nslots, uint32_t phase) {
    if (nslots < 0 || phase >= FEC_SLOTS) {
        set_err("vit_packet_fec_count: bad arguments (nslots=%lld; phase=%u, 0 ... %u)", (long long)nslots, phase, FEC_SLOTS - 1u);
        return -1;
    }
    return fec_count(nslots, phase);
}

int vit_packet_fec_sync_dev(const uint8_t* d_stream, int64_t nslots, uint32_t* d_score, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nslots < 0 || (nslots > 0 && (!d_stream || !d_score || misaligned4(d_score))))
        return bad_arg("vit_packet_fec_sync_dev: bad arguments (nslots=%lld; d_score 4-byte aligned)", (long long)nslots);
    LAUNCHCHK("FEC sync launch failed: %s", vit_launch_fec_sync(d_stream, nslots, d_score, (hipStream_t)stream));
    return VIT_OK;
}

int vit_packet_fec_dev(const uint8_t* d_stream, uint8_t* d_out, int64_t nslots, uint32_t phase, vit_fec_rec* d_fec, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    const char* why = nullptr;
    const int64_t nfec = nslots >= 0 && phase < FEC_SLOTS ? fec_count(nslots, phase) : 0;
    if (nslots < 0) why = "nslots must not be negative";
    else if (phase >= FEC_SLOTS) why = "phase must be 0 ... 102";
    else if (nslots > 0 && (!d_stream || !d_out)) why = "NULL d_stream or d_out";
    else if (nfec > 0 && (!d_fec || misaligned4(d_fec))) why = "d_fec must be 4-byte aligned and not NULL";
    else if (nfec / 20 >= 0x7FFFFFFFll) why = "too many FEC frames for one call";
    else if (nslots > 0 && d_out != d_stream) {
        const uintptr_t s = reinterpret_cast<uintptr_t>(d_stream), o = reinterpret_cast<uintptr_t>(d_out);
        const uint64_t n = (uint64_t)SLOT * (uint64_t)nslots;
        if (s < o + n && o < s + n) why = "d_out must be d_stream itself or not overlap it";
    }
    if (why) return bad_arg("vit_packet_fec_dev: bad arguments (%s; nslots=%lld phase=%u)", why, (long long)nslots, phase);
    LAUNCHCHK("FEC launch failed: %s", vit_launch_fec(d_stream, d_out, nslots, phase, nfec, d_fec, (hipStream_t)stream));
    return VIT_OK;
}

int vit_packet_fec_frame_host(uint8_t* frame, vit_fec_rec* out) {
    if (!frame || !out) return bad_arg("vit_packet_fec_frame_host: bad arguments (NULL pointer)");
    vit_fec_frame_host(frame, out);
    return VIT_OK;
}

int vit_packets_dev(const uint8_t* d_bytes, uint32_t framebytes, int64_t nframes, vit_packet_rec* d_rec, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (framebytes == 0 || framebytes > MAX_FRAMEBYTES || framebytes % SLOT || nframes < 0 ||
        (nframes > 0 && (!d_bytes || !d_rec || misaligned4(d_rec))))
        return bad_arg("vit_packets_dev: bad arguments (framebytes=%u, a multiple of 24 in 24 ... 1152; nframes=%lld; d_rec 4-byte "
                       "aligned)", framebytes, (long long)nframes);
    LAUNCHCHK("packet launch failed: %s", vit_launch_packets(d_bytes, framebytes, nframes, d_rec, (hipStream_t)stream));
    return VIT_OK;
}

namespace {

// the argument rules that vit_data_groups_dev and vit_data_groups_host share; nullptr if none is broken
const char* data_groups_why(const void* bytes, const void* rec, int64_t nslots, const void* dg, uint32_t max_groups, const void* sum,
                            const void* data, uint32_t data_capacity) {
    if (nslots < 0 || nslots > DG_MAX_SLOTS) return "nslots must be 0 ... 1<<24";
    if (nslots == 0) return nullptr;  // an empty batch touches no pointer
    if (!bytes || !rec || !sum) return "NULL bytes, records or summary";
    if (!dg && max_groups > 0) return "NULL group records with max_groups > 0";
    if (!data && data_capacity > 0) return "NULL data with data_capacity > 0";
    return nullptr;
}

}  // namespace

int vit_data_groups_dev(const uint8_t* d_bytes, const vit_packet_rec* d_rec, int64_t nslots, vit_dgroup_rec* d_dg, uint32_t max_groups,
                        vit_dgroup_summary* d_sum, uint8_t* d_data, uint32_t data_capacity, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    const char* why = data_groups_why(d_bytes, d_rec, nslots, d_dg, max_groups, d_sum, d_data, data_capacity);
    if (!why && nslots > 0 && (misaligned4(d_rec) || misaligned4(d_dg) || misaligned4(d_sum))) why = "d_rec, d_dg and d_sum must be 4-byte aligned";
    if (why) return bad_arg("vit_data_groups_dev: bad arguments (%s; nslots=%lld max_groups=%u data_capacity=%u)", why, (long long)nslots,
                            max_groups, data_capacity);
    if (nslots == 0) return VIT_OK;
    ScratchLease scratch;
    const int rc = scratch.begin(vit_data_groups_scratch(nslots), 0, (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("data group launch failed: %s", vit_launch_data_groups(d_bytes, d_rec, nslots, d_dg, max_groups, d_sum, d_data, data_capacity,
                                                                     scratch.sym<void>(), (hipStream_t)stream));
    return scratch.end();
}

int vit_data_groups_host(const uint8_t* bytes, const vit_packet_rec* rec, int64_t nslots, vit_dgroup_rec* dg, uint32_t max_groups,
                         vit_dgroup_summary* sum, uint8_t* data, uint32_t data_capacity) {
    const char* why = data_groups_why(bytes, rec, nslots, dg, max_groups, sum, data, data_capacity);
    if (why) return bad_arg("vit_data_groups_host: bad arguments (%s; nslots=%lld max_groups=%u data_capacity=%u)", why, (long long)nslots,
                            max_groups, data_capacity);
    if (nslots > 0) vit_data_groups_host_impl(bytes, rec, nslots, dg, max_groups, sum, data, data_capacity);
    return VIT_OK;
}
