// vit_api_packet.hip -- the C ABI of packet mode (include/viterbi_amd.h, "Packet mode"): argument rules and launches
// only; the kernels and the host twin are in vit_packet.hip, the format's constants in vit_packet_fmt.h.
#include <algorithm>
#include <utility>

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

// The table's rules, its layout (h_out optional) and the table as the kernels read it (tab optional); false, with the
// error text naming the entry, if a rule is broken.
bool pkt_table(const char* who, const vit_pkt_stream* h_tab, uint32_t nstreams, vit_pkt_layout* h_out, VitPktTable* tab) {
    if (!h_tab || nstreams < 1u || nstreams > VIT_PKT_MAX_STREAMS) {
        set_err("%s: bad arguments (nstreams=%u, 1 ... %u; h_tab)", who, nstreams, (unsigned)VIT_PKT_MAX_STREAMS);
        return false;
    }
    vit_pkt_layout lay = {};
    VitPktTable t = {};
    uint64_t npkt = 0, nsync = 0, nfecwg = 0;
    std::pair<uint64_t, uint32_t> order[VIT_PKT_MAX_STREAMS];  // (offset, entry)
    for (uint32_t k = 0; k < nstreams; k++) {
        const vit_pkt_stream& s = h_tab[k];
        const char* why = nullptr;
        if (s.framebytes == 0 || s.framebytes > MAX_FRAMEBYTES || s.framebytes % SLOT) why = "framebytes must be a multiple of 24 in 24 ... 1152";
        else if (s.nframes == 0) why = "nframes must be at least 1";
        else if (s.fec > VIT_PKT_FEC_SEARCH) why = "fec must be 0 (none), 1 (phase given) or 2 (phase searched)";
        else if (s.phase >= FEC_SLOTS) why = "phase must be 0 ... 102";
        else if (s.phase && s.fec != VIT_PKT_FEC_PHASE) why = "phase must be 0 unless fec is 1 (phase given)";
        else if (s.min_score && s.fec != VIT_PKT_FEC_SEARCH) why = "min_score must be 0 unless fec is 2 (phase searched)";
        else if (s.reserved) why = "reserved must be 0";
        const uint64_t S = s.framebytes / SLOT, nslots = why ? 0 : (uint64_t)s.nframes * S;
        if (!why && lay.nrec + nslots > 0x80000000ull) why = "the table holds more than 2^31 slots";
        else if (!why && s.offset + SLOT * nslots < s.offset) why = "offset + 24*nslots must fit 64 bits";
        if (why) {
            set_err("%s: bad arguments (entry %u: %s; offset=%llu framebytes=%u nframes=%u fec=%u phase=%u min_score=%u reserved=%u)", who,
                    k, why, (unsigned long long)s.offset, s.framebytes, s.nframes, s.fec, s.phase, s.min_score, s.reserved);
            return false;
        }
        lay.rec_index[k] = lay.nrec;
        lay.fec_index[k] = lay.nfecrec;
        VitPktEntry& e = t.e[k];
        e.offset = s.offset;
        e.nframes = s.nframes;
        e.nslots = (uint32_t)nslots;
        e.rec0 = (uint32_t)lay.nrec;
        e.fec0 = (uint32_t)lay.nfecrec;
        e.pkt0 = (uint32_t)npkt;
        e.sync0 = (uint32_t)nsync;
        e.fecwg0 = (uint32_t)nfecwg;
        e.S = (uint8_t)S;
        e.fec = (uint8_t)s.fec;
        e.phase = (uint8_t)s.phase;
        lay.nrec += nslots;
        lay.nfecrec += nslots / FEC_SLOTS;
        lay.bytes_end = std::max(lay.bytes_end, s.offset + SLOT * nslots);
        const uint64_t G = 64u / S;
        npkt += (s.nframes + G - 1u) / G;
        if (s.fec == VIT_PKT_FEC_SEARCH) nsync += (nslots + VIT_PKT_SYNC_CHUNK - 1u) / VIT_PKT_SYNC_CHUNK;
        // frames the stream can hold at most: at the given phase, or at phase 0 where the device chooses
        const uint64_t bound = s.fec == VIT_PKT_FEC_NONE ? 0u : (uint64_t)fec_count((int64_t)nslots, s.phase);
        nfecwg += (bound + 19u) / 20u;
        order[k] = {s.offset, k};
    }
    // (passes and workgroups are fewer than slots: they fit 32 bits with them)
    std::sort(order, order + nstreams);
    for (uint32_t j = 1; j < nstreams; j++) {
        const uint32_t a = order[j - 1u].second, b = order[j].second;
        if (h_tab[a].offset + (uint64_t)SLOT * t.e[a].nslots > h_tab[b].offset) {
            set_err("%s: bad arguments (entries %u and %u overlap: offset=%llu, %llu bytes; offset=%llu)", who, a, b,
                    (unsigned long long)h_tab[a].offset, (unsigned long long)SLOT * t.e[a].nslots, (unsigned long long)h_tab[b].offset);
            return false;
        }
    }
    t.nstreams = nstreams;
    t.npkt = (uint32_t)npkt;
    t.nsync = (uint32_t)nsync;
    t.nfecwg = (uint32_t)nfecwg;
    if (h_out) *h_out = lay;
    if (tab) *tab = t;
    return true;
}

}  // namespace

int vit_packet_table_layout(const vit_pkt_stream* h_tab, uint32_t nstreams, vit_pkt_layout* h_out) {
    if (!h_out) return bad_arg("vit_packet_table_layout: bad arguments (h_out)");
    return pkt_table("vit_packet_table_layout", h_tab, nstreams, h_out, nullptr) ? VIT_OK : VIT_ERR_ARG;
}

int vit_packet_table_dev(uint8_t* d_bytes, const vit_pkt_stream* h_tab, uint32_t nstreams, vit_pkt_stream_rec* d_srec, vit_fec_rec* d_fec,
                         vit_packet_rec* d_rec, uint32_t* d_score, void* stream) {
    static const char* const who = "vit_packet_table_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    vit_pkt_layout lay;
    VitPktTable tab;
    if (!pkt_table(who, h_tab, nstreams, &lay, &tab)) return VIT_ERR_ARG;
    const char* why = nullptr;
    if (!d_bytes || !d_srec || !d_rec) why = "NULL d_bytes, d_srec or d_rec";
    else if (misaligned4(d_srec) || misaligned4(d_fec) || misaligned4(d_rec) || misaligned4(d_score)) why = "d_srec, d_fec, d_rec and d_score must be 4-byte aligned";
    else if (!d_fec && lay.nfecrec > 0) why = "d_fec may be NULL only when the layout's nfecrec is 0";
    if (why) return bad_arg("%s: bad arguments (%s)", who, why);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t min_score[VIT_PKT_MAX_STREAMS];
    for (uint32_t k = 0; k < nstreams; k++) min_score[k] = h_tab[k].min_score;
    // Nothing below waits for the device or copies from it: a memset and four kernels on `stream`, and around them the
    // scratch lease's event (a wait and a record on the stream) when the scores live in the thread's scratch.
    const bool search = tab.nsync > 0, own_scores = search && !d_score;
    ScratchLease scratch;
    if (own_scores) {
        const int rc = scratch.begin((size_t)nstreams * FEC_SLOTS * sizeof(uint32_t), 0, s);
        if (rc != VIT_OK) return rc;
        d_score = scratch.sym<uint32_t>();
    }
    if (d_score) LAUNCHCHK("packet table sync launch failed: %s", vit_launch_pkt_table_sync(d_bytes, tab, d_score, s));
    LAUNCHCHK("packet table pick launch failed: %s", vit_launch_pkt_table_pick(tab, d_score, min_score, d_srec, s));
    LAUNCHCHK("packet table FEC launch failed: %s", vit_launch_pkt_table_fec(d_bytes, tab, d_srec, d_fec, s));
    LAUNCHCHK("packet table packets launch failed: %s", vit_launch_pkt_table_packets(d_bytes, tab, d_rec, s));
    return own_scores ? scratch.end() : VIT_OK;
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

namespace {

// The data group table's rules, its layout (h_out optional) and the table as the kernels read it, without its geometry
// (tab optional); false, with the error text naming the entry, if a rule is broken.
bool dg_table(const char* who, const vit_dg_stream* h_tab, uint32_t nstreams, vit_dg_layout* h_out, VitDgTable* tab) {
    if (!h_tab || nstreams < 1u || nstreams > VIT_DG_MAX_STREAMS) {
        set_err("%s: bad arguments (nstreams=%u, 1 ... %u; h_tab)", who, nstreams, (unsigned)VIT_DG_MAX_STREAMS);
        return false;
    }
    vit_dg_layout lay = {};
    VitDgTable t = {};
    uint64_t slots = 0;
    for (uint32_t k = 0; k < nstreams; k++) {
        const vit_dg_stream& s = h_tab[k];
        const char* why = nullptr;
        if (s.nslots < 1u || s.nslots > DG_MAX_SLOTS) why = "nslots must be 1 ... 1<<24";
        else if (s.records_only > 1u) why = "records_only must be 0 or 1";
        else if (s.records_only && s.data_capacity) why = "data_capacity must be 0 with records_only 1";
        else if (s.offset + (uint64_t)SLOT * s.nslots < s.offset) why = "offset + 24*nslots must fit 64 bits";
        else if (s.rec_index + s.nslots < s.rec_index) why = "rec_index + nslots must fit 64 bits";
        else if (slots + s.nslots > (1ull << 26)) why = "the table holds more than 1<<26 slots (16 bytes of scratch per slot: 1 GiB)";
        else if (lay.ndg > 0xFFFFFFFFull) why = "dg_index must stay below 2^32";
        else if (lay.data_bytes > 0xFFFFFFFFull) why = "data_offset must stay below 2^32";
        if (why) {
            set_err("%s: bad arguments (entry %u: %s; offset=%llu rec_index=%llu nslots=%u max_groups=%u data_capacity=%u records_only=%u)",
                    who, k, why, (unsigned long long)s.offset, (unsigned long long)s.rec_index, s.nslots, s.max_groups, s.data_capacity,
                    s.records_only);
            return false;
        }
        lay.dg_index[k] = lay.ndg;
        lay.data_offset[k] = lay.data_bytes;
        VitDgEntry& e = t.e[k];
        e.offset = s.offset;
        e.rec0 = s.rec_index;
        e.nslots = s.nslots;
        e.max_groups = s.max_groups;
        e.capacity = s.data_capacity;
        e.has_data = s.records_only ? 0u : 1u;
        e.dg0 = (uint32_t)lay.ndg;
        e.data0 = (uint32_t)lay.data_bytes;
        slots += s.nslots;
        lay.ndg += s.max_groups;
        lay.data_bytes += ((uint64_t)s.data_capacity + DG_ALIGN - 1u) & ~(uint64_t)(DG_ALIGN - 1u);
        lay.bytes_end = std::max(lay.bytes_end, s.offset + (uint64_t)SLOT * s.nslots);
        lay.rec_end = std::max(lay.rec_end, s.rec_index + s.nslots);
    }
    t.nstreams = nstreams;
    if (h_out) *h_out = lay;
    if (tab) *tab = t;
    return true;
}

}  // namespace

int vit_data_groups_table_layout(const vit_dg_stream* h_tab, uint32_t nstreams, vit_dg_layout* h_out) {
    if (!h_out) return bad_arg("vit_data_groups_table_layout: bad arguments (h_out)");
    return dg_table("vit_data_groups_table_layout", h_tab, nstreams, h_out, nullptr) ? VIT_OK : VIT_ERR_ARG;
}

int vit_data_groups_table_dev(const uint8_t* d_bytes, const vit_packet_rec* d_rec, const vit_dg_stream* h_tab, uint32_t nstreams,
                              vit_dgroup_rec* d_dg, vit_dgroup_summary* d_sum, uint8_t* d_data, void* stream) {
    static const char* const who = "vit_data_groups_table_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    vit_dg_layout lay;
    VitDgTable tab;
    if (!dg_table(who, h_tab, nstreams, &lay, &tab)) return VIT_ERR_ARG;
    bool wants_data = false;
    for (uint32_t k = 0; k < nstreams; k++) wants_data = wants_data || (tab.e[k].has_data && tab.e[k].capacity > 0);
    const char* why = nullptr;
    if (!d_bytes || !d_rec || !d_sum) why = "NULL d_bytes, d_rec or d_sum";
    else if (!d_dg && lay.ndg > 0) why = "d_dg may be NULL only when the layout's ndg is 0";
    else if (!d_data && wants_data) why = "d_data may be NULL only when no entry with records_only 0 has a data_capacity";
    else if (misaligned4(d_rec) || misaligned4(d_dg) || misaligned4(d_sum)) why = "d_rec, d_dg and d_sum must be 4-byte aligned";
    if (why) return bad_arg("%s: bad arguments (%s)", who, why);
    if (!d_data)  // every stream as with d_data NULL
        for (uint32_t k = 0; k < nstreams; k++) tab.e[k].has_data = 0;
    // Nothing below waits for the device or copies from it: a memset and the kernels on `stream`, between the scratch
    // lease's wait and record.
    const hipStream_t s = (hipStream_t)stream;
    ScratchLease scratch;
    const int rc = scratch.begin(vit_dg_table_geometry(&tab), 0, s);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("data group table launch failed: %s", vit_launch_data_groups_table(d_bytes, d_rec, tab, d_dg, d_sum, d_data, scratch.sym<void>(), s));
    return scratch.end();
}
