// vit_api_decode.hip -- the C ABI around the decoder (include/viterbi_amd.h): kernel choice and the one decode dispatch,
// the batched decode entry points (u8, u32, variable length, checked, punctured), the chains behind the decoder (energy
// dispersal, FIB CRC, FIC, DAB+ superframes and access units, fire code, RS) and MSC time de-interleaving in front of it.
// Argument rules and launches only: vit_host.h has what the units of the C ABI share.
#include <algorithm>
#include <cstdlib>

#include "vit_host.h"

#ifdef VIT_WITH_PK8
static bool pk8_default() {
    static const bool on = [] {
        const char* e = getenv("VITERBI_AMD_PK8");
        return e ? atoi(e) != 0 : false;
    }();
    return on;
}
#else  // the experiment is not compiled in: the launcher's names exist, the kernel does not
static bool pk8_default() { return false; }
bool vit_pk8_supported(uint32_t) { return false; }
hipError_t vit_launch_pk8(const void*, bool, uint8_t*, const vit_frame_desc*, uint32_t, uint32_t, int64_t, hipStream_t, bool) {
    return hipErrorNotSupported;
}
#endif

int pick_kernel(int choice, uint32_t max_framebits, int64_t nframes) {
    if (choice == K_WAVE || choice == K_LATENCY) return choice;
    if (choice == K_PACKED8) return vit_pk8_supported(max_framebits) ? K_PACKED8 : -1;
    if (choice == K_AUTO && nframes <= VIT_LAT_MAX_FRAMES) {  // small launch: does it fit the latency kernel's residency?
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && nframes <= vit_lat_capacity(max_framebits, dev)) return K_LATENCY;
    }
    return vit_pk_supported(max_framebits) ? K_PACKED : (choice == K_PACKED ? -1 : K_WAVE);
}
// the kernel pick_kernel chose (k): the packed kernel's opt-in promotion to the 8-frame experiment, and the launch
static int launch_picked(int k, DecodeMode mode, const void* sym, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                         uint32_t framebits, uint32_t max_framebits, int64_t nframes, hipStream_t s) {
    if (k < 0) return bad_arg("packed kernel does not support framebits=%u", max_framebits);
    if (k == K_PACKED && !d_desc && pk8_default() && vit_pk8_supported(max_framebits)) k = K_PACKED8;
    LAUNCHCHK("kernel launch failed: %s",
              k == K_PACKED8   ? vit_launch_pk8(sym, sym32, d_out, d_desc, framebits, max_framebits, nframes, s, mode.ge)
              : k == K_PACKED  ? vit_launch_pk(sym, sym32, d_out, d_desc, framebits, max_framebits, nframes, s, mode.ge)
              : k == K_LATENCY ? vit_launch_lat(sym, sym32, d_out, d_desc, framebits, max_framebits, nframes, s, nullptr, 0, mode.ge)
                               : vit_launch_wave((const uint8_t*)sym, d_out, d_desc, framebits, max_framebits, nframes, s, mode.ge));
    return VIT_OK;
}
int launch_decode(DecodeMode mode, const void* symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                  uint32_t framebits, uint32_t max_framebits, int64_t nframes, hipStream_t s) {
    const int k = pick_kernel(mode.kernel, max_framebits, nframes);
    const bool in_place = (k == K_PACKED || k == K_PACKED8 || k == K_LATENCY) && (reinterpret_cast<uintptr_t>(symbols) & 15u) == 0;
    if (!sym32 || in_place)  // no scratch, no extra launch
        return launch_picked(k, mode, symbols, sym32, d_out, d_desc, framebits, max_framebits, nframes, s);
    // the narrowing fallback (uniform batches only: frame f's symbols at f * 4 * (framebits + 6))
    const int64_t nsym = nframes * 4 * ((int64_t)framebits + VIT_TAIL);
    ScratchLease scratch;
    int rc = scratch.begin((size_t)nsym, 0, s);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("pack launch failed: %s", vit_launch_pack((const uint32_t*)symbols, scratch.sym<uint8_t>(), nsym, s));
    rc = launch_picked(k, mode, scratch.sym<uint8_t>(), false, d_out, d_desc, framebits, max_framebits, nframes, s);
    return rc != VIT_OK ? rc : scratch.end();
}

bool ring_check_base(const char* who, const vit_cif_ring* ring, const char* null_fmt) {
    if (!ring || !ring->d_base) {
        set_err(null_fmt, who);
        return false;
    }
    if (ring->first_row >= ring->nrows) {
        set_err("%s: bad arguments (first_row %u >= nrows %u)", who, ring->first_row, ring->nrows);
        return false;
    }
    return true;
}
bool ring_check_cols(const char* who, const vit_cif_ring* ring, uint64_t col, uint64_t ncols) {
    if (col > ring->row_bytes || ncols > ring->row_bytes - col) {
        set_err("%s: bad arguments (columns [%llu, %llu + %llu) outside row_bytes %llu)", who, (unsigned long long)col,
                (unsigned long long)col, (unsigned long long)ncols, (unsigned long long)ring->row_bytes);
        return false;
    }
    return true;
}

extern "C" {

int vit_pack_symbols_dev(const uint32_t* d_symbols_u32, uint8_t* d_symbols_u8, int64_t nsym, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nsym < 0 || (nsym > 0 && (!d_symbols_u32 || !d_symbols_u8))) return bad_arg("vit_pack_symbols_dev: bad arguments");
    LAUNCHCHK("pack launch failed: %s", vit_launch_pack(d_symbols_u32, d_symbols_u8, nsym, (hipStream_t)stream));
    return VIT_OK;
}

int vit_decode_batch_dev(const uint8_t* d_symbols_u8, uint8_t* d_decoded, uint32_t framebits, int64_t nframes,
                         void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && (!d_symbols_u8 || !d_decoded)))
        return bad_arg("vit_decode_batch_dev: bad arguments (framebits=%u nframes=%lld)", framebits, (long long)nframes);
    if (framebits == 0 || nframes == 0) return VIT_OK;
    return launch_decode(decode_mode(), d_symbols_u8, false, d_decoded, nullptr, framebits, framebits, nframes,
                         (hipStream_t)stream);
}

int vit_decode_batch_dev_u32(const uint32_t* d_symbols_u32, uint8_t* d_decoded, uint32_t framebits,
                             int64_t nframes, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && (!d_symbols_u32 || !d_decoded)))
        return bad_arg("vit_decode_batch_dev_u32: bad arguments");
    if (framebits == 0 || nframes == 0) return VIT_OK;
    return launch_decode(decode_mode(), d_symbols_u32, true, d_decoded, nullptr, framebits, framebits, nframes, (hipStream_t)stream);
}

int vit_decode_varlen_dev(const uint8_t* d_symbols_u8, uint8_t* d_decoded, const vit_frame_desc* d_desc,
                          int64_t nframes, uint32_t max_framebits, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(max_framebits) || nframes < 0 ||
        (nframes > 0 && (!d_symbols_u8 || !d_decoded || !d_desc)))
        return bad_arg("vit_decode_varlen_dev: bad arguments");
    if (nframes == 0 || max_framebits == 0) return VIT_OK;
    return launch_decode(decode_mode(), d_symbols_u8, false, d_decoded, d_desc, 0, max_framebits, nframes, (hipStream_t)stream);
}

int vit_decode_varlen_dev_checked(const uint8_t* d_symbols_u8, uint64_t sym_bytes, uint8_t* d_decoded, uint64_t out_bytes,
                                  const vit_frame_desc* d_desc, int64_t nframes, uint32_t max_framebits, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(max_framebits) || nframes < 0 ||
        (nframes > 0 && (!d_symbols_u8 || !d_decoded || !d_desc)))
        return bad_arg("vit_decode_varlen_dev_checked: bad arguments");
    if (nframes == 0 || max_framebits == 0) return VIT_OK;
    // the checked copy lives in this thread's descriptor scratch
    ScratchLease scratch;
    int rc = scratch.begin(0, (size_t)nframes * sizeof(vit_frame_desc), (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("descriptor check launch failed: %s",
              vit_check_descs_launch(d_desc, scratch.desc(), nframes, sym_bytes, out_bytes, (hipStream_t)stream));
    rc = launch_decode(decode_mode(), d_symbols_u8, false, d_decoded, scratch.desc(), 0, max_framebits, nframes, (hipStream_t)stream);
    return rc != VIT_OK ? rc : scratch.end();
}

int64_t vit_punctured_length(const vit_punct_profile* p, uint32_t framebits) {
    return vit_punct_length_host(p, framebits, nullptr, nullptr);
}

// The argument rules of a CIF ring (include/viterbi_amd.h, vit_cif_ring) for a call of nframes > 0 frames that reads
// ncols columns from col: false (with the error text set) if one is broken.
static bool check_ring(const char* who, const vit_cif_ring* ring, uint64_t col, uint64_t ncols, int64_t nframes) {
    if (!ring_check_base(who, ring, "%s: bad arguments (NULL ring or d_base)")) return false;
    if ((uint64_t)nframes + 15u > ring->nrows) {
        set_err("%s: bad arguments (%lld frames need %lld distinct rows, the ring has %u)", who, (long long)nframes,
                (long long)nframes + 15, ring->nrows);
        return false;
    }
    return ring_check_cols(who, ring, col, ncols);
}

// Punctured input: the transmitted symbols are expanded into this thread's scratch buffer on the caller's current
// device (the one the u32 path narrows into; vit_punct.hip), and the unchanged decoders read them from there.
// Shared by vit_decode_punctured_dev and the chains after the decoder: profile == NULL decodes depunctured u8 symbols
// directly (no expansion, no scratch).  The caller has checked framebits (> 0), nframes (> 0) and d_out; the profile
// and d_in are checked here, before anything is launched.
// ring != NULL (the *_ti_dev calls, profile required): the transmitted symbols come from columns [col, col + P) of a CIF
// ring instead of d_in, and the expansion de-interleaves them (vit_ti.hip).
static int decode_maybe_punctured(const char* who, const uint8_t* d_in, uint8_t* d_out, uint32_t framebits, int64_t nframes,
                                  const vit_punct_profile* profile, uint8_t erasure, hipStream_t stream,
                                  const vit_cif_ring* ring = nullptr, uint64_t col = 0) {
    if (!profile) {
        if (!d_in) return bad_arg("%s: bad arguments (d_in)", who);
        return launch_decode(decode_mode(), d_in, false, d_out, nullptr, framebits, framebits, nframes, stream);
    }
    const int64_t P = vit_punctured_length(profile, framebits);
    if (P < 0)
        return bad_arg("%s: invalid puncturing profile, or its steps do not sum to framebits+6 = %u", who, framebits + VIT_TAIL);
    if (ring) {
        if (!check_ring(who, ring, col, (uint64_t)P, nframes)) return VIT_ERR_ARG;
    } else if (P > 0 && !d_in) {  // (a profile that punctures everything reads no input)
        set_err("%s: bad arguments (d_punct)", who);
        return VIT_ERR_ARG;
    }
    ScratchLease scratch;
    int rc = scratch.begin((size_t)nframes * 4u * (framebits + VIT_TAIL), 0, stream);
    if (rc != VIT_OK) return rc;
    uint8_t* d_sym8 = scratch.sym<uint8_t>();
    LAUNCHCHK("depuncture launch failed: %s",
              ring ? vit_launch_depunct_ti(*ring, col, d_sym8, framebits, nframes, profile, erasure, stream)
                   : vit_launch_depunct(d_in, d_sym8, framebits, nframes, profile, erasure, stream));
    rc = launch_decode(decode_mode(), d_sym8, false, d_out, nullptr, framebits, framebits, nframes, stream);
    return rc != VIT_OK ? rc : scratch.end();
}

int vit_decode_punctured_dev(const uint8_t* d_punct, uint8_t* d_decoded, uint32_t framebits, int64_t nframes,
                             const vit_punct_profile* profile, uint8_t erasure, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && !d_decoded))
        return bad_arg("vit_decode_punctured_dev: bad arguments (framebits=%u nframes=%lld)", framebits, (long long)nframes);
    if (framebits == 0 || nframes == 0) return VIT_OK;
    if (!profile) {  // (NULL means "not punctured" only to the chains after the decoder)
        set_err("vit_decode_punctured_dev: invalid puncturing profile, or its steps do not sum to framebits+6 = %u",
                framebits + VIT_TAIL);
        return VIT_ERR_ARG;
    }
    return decode_maybe_punctured("vit_decode_punctured_dev", d_punct, d_decoded, framebits, nframes, profile, erasure,
                                  (hipStream_t)stream);
}

int vit_decode_punctured_varlen_dev(const uint8_t* d_punct, uint64_t sym_bytes, uint8_t* d_decoded, uint64_t out_bytes,
                                    const vit_frame_desc* d_desc, int64_t nframes, uint32_t max_framebits,
                                    const vit_punct_profile* d_profiles, uint32_t nprofiles, uint8_t erasure, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(max_framebits) || nframes < 0 ||
        (nframes > 0 && (!d_punct || !d_decoded || !d_desc || (nprofiles > 0 && !d_profiles))))
        return bad_arg("vit_decode_punctured_varlen_dev: bad arguments");
    if (nframes == 0 || max_framebits == 0) return VIT_OK;
    // frame i's expanded symbols go to slot i of this thread's scratch buffer (no scan over the lengths), its
    // internal descriptor to the thread's descriptor scratch (the checked path's copy).  The sort and the long-frame
    // kernel keep their own scratch (vit_pk.hip).
    const size_t slot = 4u * ((size_t)max_framebits + VIT_TAIL);
    ScratchLease scratch;
    int rc = scratch.begin((size_t)nframes * slot, (size_t)nframes * sizeof(vit_frame_desc), (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("depuncture launch failed: %s",
              vit_launch_depunct_varlen(d_punct, sym_bytes, out_bytes, d_desc, nframes, max_framebits, d_profiles, nprofiles, erasure,
                                        scratch.sym<uint8_t>(), scratch.desc(), (hipStream_t)stream));
    rc = launch_decode(decode_mode(), scratch.sym<uint8_t>(), false, d_decoded, scratch.desc(), 0, max_framebits, nframes,
                       (hipStream_t)stream);
    return rc != VIT_OK ? rc : scratch.end();
}

// ---- after the decoder: energy dispersal, FIB CRC, DAB+ fire code (vit_dab.hip) ----------------------------------
int64_t vit_energy_dispersal_prbs(uint8_t* h_out, uint32_t framebits) {
    if (!valid_framebits(framebits) || !h_out) {
        set_err("vit_energy_dispersal_prbs: bad arguments (framebits=%u)", framebits);
        return -1;
    }
    return vit_prbs_bytes_host(h_out, framebits);
}

int vit_energy_dispersal_dev(uint8_t* d_bytes, uint32_t framebits, int64_t nframes, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && !d_bytes))
        return bad_arg("vit_energy_dispersal_dev: bad arguments (framebits=%u nframes=%lld)", framebits, (long long)nframes);
    LAUNCHCHK("energy dispersal launch failed: %s", vit_launch_disperse(d_bytes, framebits, nframes, (hipStream_t)stream));
    return VIT_OK;
}

int vit_energy_dispersal_varlen_dev(uint8_t* d_bytes, uint64_t out_bytes, const vit_frame_desc* d_desc, int64_t nframes,
                                    void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nframes < 0 || (nframes > 0 && (!d_bytes || !d_desc))) return bad_arg("vit_energy_dispersal_varlen_dev: bad arguments");
    LAUNCHCHK("energy dispersal launch failed: %s",
              vit_launch_disperse_varlen(d_bytes, out_bytes, d_desc, nframes, (hipStream_t)stream));
    return VIT_OK;
}

int vit_fib_crc_dev(const uint8_t* d_fibs, int64_t nfibs, uint8_t* d_ok, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nfibs < 0 || (nfibs > 0 && (!d_fibs || !d_ok))) return bad_arg("vit_fib_crc_dev: bad arguments");
    LAUNCHCHK("FIB CRC launch failed: %s",
              vit_launch_fibs(const_cast<uint8_t*>(d_fibs), nfibs, 1, false, d_ok, (hipStream_t)stream));
    return VIT_OK;
}

int vit_decode_fic_dev(const uint8_t* d_in, uint8_t* d_fibs, uint8_t* d_fib_ok, uint32_t framebits, int64_t nframes,
                       const vit_punct_profile* profile, uint8_t erasure, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (framebits == 0 || framebits % 256u != 0 || framebits > VIT_MAX_FRAMEBITS || nframes < 0 ||
        (nframes > 0 && (!d_fibs || !d_fib_ok)))
        return bad_arg("vit_decode_fic_dev: bad arguments (framebits=%u, a multiple of 256 up to 9216; nframes=%lld)", framebits,
                       (long long)nframes);
    if (nframes == 0) return VIT_OK;
    int rc = decode_maybe_punctured("vit_decode_fic_dev", d_in, d_fibs, framebits, nframes, profile, erasure,
                                    (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    const uint32_t fpf = framebits / 256u;
    LAUNCHCHK("FIB post-pass launch failed: %s",
              vit_launch_fibs(d_fibs, nframes * fpf, fpf, true, d_fib_ok, (hipStream_t)stream));
    return VIT_OK;
}

// The DAB+ chain of both entry points; from_ring: the *_ti_dev form, which reads `ring` (required, as the profile is)
// instead of d_in.
static int dabplus_chain(const char* who, const uint8_t* d_in, bool from_ring, const vit_cif_ring* ring, uint64_t col,
                         const vit_punct_profile* profile, uint8_t erasure, uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret,
                         uint8_t* d_fire_ok, uint32_t RSDims, int64_t nsf, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (RSDims == 0 || 192ull * RSDims > VIT_MAX_FRAMEBITS || nsf < 0 || (nsf > 0 && (!d_work || !d_rs_out || !d_ret)))
        return bad_arg("%s: bad arguments (RSDims=%u, 1 ... 48; nsf=%lld)", who, RSDims, (long long)nsf);
    if (nsf == 0) return VIT_OK;
    if (from_ring && !ring) return bad_arg("%s: bad arguments (NULL ring)", who);
    if (from_ring && !profile) return bad_arg("%s: a puncturing profile is required", who);
    int rc = decode_maybe_punctured(who, d_in, d_work, 192u * RSDims, 5 * nsf, profile, erasure, (hipStream_t)stream, ring,
                                    col);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("DAB+ post-pass launch failed: %s", vit_launch_dabplus_post(d_work, RSDims, nsf, d_fire_ok, (hipStream_t)stream));
    LAUNCHCHK("rs launch failed: %s", rs_launch(d_work, d_rs_out, d_ret, RSDims, nsf, (hipStream_t)stream));
    return VIT_OK;
}

int vit_dabplus_punctured_superframes_dev(const uint8_t* d_in, const vit_punct_profile* profile, uint8_t erasure,
                                          uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret, uint8_t* d_fire_ok,
                                          uint32_t RSDims, int64_t nsf, void* stream) {
    return dabplus_chain("vit_dabplus_punctured_superframes_dev", d_in, false, nullptr, 0, profile, erasure, d_work, d_rs_out,
                         d_ret, d_fire_ok, RSDims, nsf, stream);
}

// ---- DAB+ access units: superframe header and AU CRCs, per-frame fire code (vit_dab.hip) ----------------------------
int vit_dabplus_aus_dev(const uint8_t* d_sf, uint64_t sf_stride, uint32_t RSDims, int64_t nsf, const int32_t* d_ret,
                        vit_au_table* d_au, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (RSDims == 0 || RSDims > 48u || nsf < 0 || sf_stride < 110ull * RSDims ||
        (nsf > 0 && (!d_sf || !d_au || (reinterpret_cast<uintptr_t>(d_au) & 3u))))
        return bad_arg("vit_dabplus_aus_dev: bad arguments (RSDims=%u, 1 ... 48; nsf=%lld; sf_stride=%llu, >= 110*RSDims; d_au "
                       "4-byte aligned)", RSDims, (long long)nsf, (unsigned long long)sf_stride);
    LAUNCHCHK("access unit launch failed: %s", vit_launch_aus(d_sf, sf_stride, RSDims, nsf, d_ret, d_au, (hipStream_t)stream));
    return VIT_OK;
}

int vit_dabplus_aus_host(const uint8_t* h_sf, uint32_t RSDims, vit_au_table* h_out) {
    if (!h_sf || !h_out || RSDims == 0 || RSDims > 48u)
        return bad_arg("vit_dabplus_aus_host: bad arguments (RSDims=%u, 1 ... 48)", RSDims);
    vit_au_table_host(h_sf, RSDims, h_out);
    return VIT_OK;
}

int vit_fire_code_dev(const uint8_t* d_bytes, uint64_t stride, int64_t n, uint8_t* d_ok, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (n < 0 || (n > 0 && (!d_bytes || !d_ok))) return bad_arg("vit_fire_code_dev: bad arguments (n=%lld)", (long long)n);
    LAUNCHCHK("fire code launch failed: %s", vit_launch_fire(d_bytes, stride, n, d_ok, (hipStream_t)stream));
    return VIT_OK;
}

// ---- from the CIF stream: MSC time de-interleaving (vit_ti.hip) ---------------------------------------------------
int vit_time_deinterleave_dev(const vit_cif_ring* ring, uint64_t col, uint32_t ncols, uint8_t* d_out, int64_t nframes,
                              void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nframes < 0 || (nframes > 0 && ncols > 0 && !d_out))
        return bad_arg("vit_time_deinterleave_dev: bad arguments (nframes=%lld)", (long long)nframes);
    if (nframes == 0) return VIT_OK;
    if (!check_ring("vit_time_deinterleave_dev", ring, col, ncols, nframes)) return VIT_ERR_ARG;
    LAUNCHCHK("time de-interleave launch failed: %s",
              vit_launch_time_deinterleave(*ring, col, ncols, d_out, nframes, (hipStream_t)stream));
    return VIT_OK;
}

int vit_decode_punctured_ti_dev(const vit_cif_ring* ring, uint64_t col, uint8_t* d_decoded, uint32_t framebits,
                                int64_t nframes, const vit_punct_profile* profile, uint8_t erasure, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!valid_framebits(framebits) || nframes < 0 || (nframes > 0 && framebits > 0 && !d_decoded))
        return bad_arg("vit_decode_punctured_ti_dev: bad arguments (framebits=%u nframes=%lld)", framebits, (long long)nframes);
    if (framebits == 0 || nframes == 0) return VIT_OK;
    if (!ring) return bad_arg("vit_decode_punctured_ti_dev: bad arguments (NULL ring)");
    if (!profile) return bad_arg("vit_decode_punctured_ti_dev: a puncturing profile is required");
    return decode_maybe_punctured("vit_decode_punctured_ti_dev", nullptr, d_decoded, framebits, nframes, profile, erasure,
                                  (hipStream_t)stream, ring, col);
}

int vit_dabplus_ti_superframes_dev(const vit_cif_ring* ring, uint64_t col, const vit_punct_profile* profile, uint8_t erasure,
                                   uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret, uint8_t* d_fire_ok, uint32_t RSDims,
                                   int64_t nsf, void* stream) {
    return dabplus_chain("vit_dabplus_ti_superframes_dev", nullptr, true, ring, col, profile, erasure, d_work, d_rs_out, d_ret,
                         d_fire_ok, RSDims, nsf, stream);
}

void vit_sort_descs(vit_frame_desc* h_desc, int64_t nframes) {
    if (!h_desc || nframes <= 1) return;
    std::stable_sort(h_desc, h_desc + nframes,
                     [](const vit_frame_desc& a, const vit_frame_desc& b) { return a.framebits > b.framebits; });
}

int vit_rs_batch_dev(const uint8_t* d_p, uint8_t* d_out, int32_t* d_ret, uint32_t RSDims, int64_t nsf, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (nsf < 0 || (nsf > 0 && RSDims > 0 && (!d_p || !d_out || !d_ret)) || RSDims > 65535u)
        return bad_arg("vit_rs_batch_dev: bad arguments");
    if (nsf == 0) return VIT_OK;
    if (RSDims == 0) {  // zero columns: the reference's loop does not run, returns 0
        LAUNCHCHK("memset: %s", hipMemsetAsync(d_ret, 0, (size_t)nsf * sizeof(int32_t), (hipStream_t)stream));
        return VIT_OK;
    }
    LAUNCHCHK("rs launch failed: %s", rs_launch(d_p, d_out, d_ret, RSDims, nsf, (hipStream_t)stream));
    return VIT_OK;
}

int vit_dabplus_superframes_dev(const uint8_t* d_symbols_u8, uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret,
                                uint32_t RSDims, int64_t nsf, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    const uint64_t framebits = 192ull * RSDims;  // 24 ms frame of an RSDims*8 kbit/s sub-channel
    if (RSDims == 0 || framebits > VIT_MAX_FRAMEBITS || nsf < 0 ||
        (nsf > 0 && (!d_symbols_u8 || !d_work || !d_rs_out || !d_ret)))
        return bad_arg("vit_dabplus_superframes_dev: bad arguments (RSDims=%u)", RSDims);
    if (nsf == 0) return VIT_OK;
    int rc = launch_decode(decode_mode(), d_symbols_u8, false, d_work, nullptr, (uint32_t)framebits, (uint32_t)framebits, 5 * nsf,
                           (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    return vit_rs_batch_dev(d_work, d_rs_out, d_ret, RSDims, nsf, stream);
}

}  // extern "C"
