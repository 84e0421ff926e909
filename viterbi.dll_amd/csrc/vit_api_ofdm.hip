// vit_api_ofdm.hip -- the C ABI of the receiver front (include/viterbi_amd.h): bins, twiddles and the NCO table, demapping,
// FFT and demodulation, fine synchronisation, sample conversion, rate conversion, first acquisition and transmitter
// identification.  Argument rules and launches only: vit_host.h has what the units of the C ABI share.
#include <climits>
#include <cmath>

#include "vit_host.h"

static bool valid_nfft(uint32_t nfft) { return nfft >= 64u && nfft <= 8192u && (nfft & (nfft - 1u)) == 0; }

extern "C" {

// ---- from the FFT: differential demodulation, frequency de-interleaving, demapping (vit_ofdm.hip) ------------------
int64_t vit_freq_interleave_bins(uint32_t nfft, uint16_t* h_bins) {
    const int64_t n = vit_freq_bins_host(nfft, h_bins);
    if (n < 0) set_err("vit_freq_interleave_bins: bad arguments (nfft=%u, one of 256, 512, 1024, 2048)", nfft);
    return n;
}

// the rules of vit_ofdm_demap_dev for where the soft bytes go and what they are made from (shared with vit_ofdm_demod_dev)
static int ofdm_check_outputs(const char* who, const vit_ofdm_shape* shape, float gain, int64_t nframes, const uint8_t* d_fic,
                              const vit_cif_ring* ring, uint64_t col) {
    if (!d_fic && !ring) return bad_arg("%s: bad arguments (d_fic and ring both NULL)", who);
    const vit_ofdm_shape& sh = *shape;
    if (!valid_nfft(sh.nfft) || sh.ncarriers == 0 || sh.ncarriers > sh.nfft ||
        sh.nsyms <= sh.fic_syms || sh.cifs == 0 || (sh.nsyms - 1u - sh.fic_syms) % sh.cifs != 0)
        return bad_arg("%s: bad arguments (shape {nfft=%u ncarriers=%u nsyms=%u fic_syms=%u cifs=%u})", who, sh.nfft, sh.ncarriers,
                       sh.nsyms, sh.fic_syms, sh.cifs);
    if (!(gain > 0.0f && gain <= 65536.0f)) {  // false for NaN
        set_err("%s: bad arguments (gain %g, 0 < gain <= 65536)", who, (double)gain);
        return VIT_ERR_ARG;
    }
    if (ring) {
        const uint64_t per_bytes = (uint64_t)((sh.nsyms - 1u - sh.fic_syms) / sh.cifs) * 2u * sh.ncarriers;
        if (!ring_check_base(who, ring, "%s: bad arguments (NULL d_base)")) return VIT_ERR_ARG;
        if ((uint64_t)nframes > ring->nrows / sh.cifs)
            return bad_arg("%s: bad arguments (%lld frames of %u CIFs need distinct rows, the ring has %u)", who, (long long)nframes,
                           sh.cifs, ring->nrows);
        if (!ring_check_cols(who, ring, col, per_bytes)) return VIT_ERR_ARG;
    }
    return VIT_OK;
}

// the rules of vit_soft_rule (after VIT_ERR_NO_DEVICE): on VIT_OK *gain is the rule's gain, still to pass ofdm_check_outputs
static int ofdm_check_soft(const char* who, const vit_soft_rule* soft, const float* d_level, float* gain) {
    if (!soft) return bad_arg("%s: bad arguments (NULL soft)", who);
    if (soft->rule != VIT_SOFT_PER_CARRIER && soft->rule != VIT_SOFT_PER_SYMBOL)
        return bad_arg("%s: bad arguments (rule %u, VIT_SOFT_PER_CARRIER or VIT_SOFT_PER_SYMBOL)", who, soft->rule);
    if (soft->rule == VIT_SOFT_PER_CARRIER && d_level)
        return bad_arg("%s: bad arguments (d_level needs VIT_SOFT_PER_SYMBOL: the per-carrier rule forms no level)", who);
    if (soft->rule == VIT_SOFT_PER_SYMBOL && !(soft->gain >= 0x1p-24f && soft->gain <= 65536.0f)) {  // false for NaN
        set_err("%s: bad arguments (gain %g, 2^-24 <= gain <= 65536 for VIT_SOFT_PER_SYMBOL)", who, (double)soft->gain);
        return VIT_ERR_ARG;
    }
    if (((uintptr_t)d_level & 3u) != 0) return bad_arg("%s: bad arguments (d_level must be 4-byte aligned)", who);
    *gain = soft->gain;
    return VIT_OK;
}

static int ofdm_demap(const char* who, const float* d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t* d_bins,
                      const vit_ofdm_shape* shape, float gain, uint32_t rule, int64_t nframes, uint8_t* d_fic,
                      const vit_cif_ring* ring, uint64_t col, float* d_level, void* stream) {
    if (!d_fft || !d_bins || !shape || nframes < 0)
        return bad_arg("%s: bad arguments (NULL d_fft, d_bins or shape, or nframes=%lld < 0)", who, (long long)nframes);
    const vit_ofdm_shape& sh = *shape;
    if (ofdm_check_outputs(who, shape, gain, nframes, d_fic, ring, col) != VIT_OK) return VIT_ERR_ARG;
    if (((uintptr_t)d_fft & 15u) != 0 || (sym_stride & 1u) != 0 || (frame_stride & 1u) != 0 || sym_stride < sh.nfft)
        return bad_arg("%s: bad arguments (d_fft must be 16-byte aligned, sym_stride %llu and frame_stride %llu even, sym_stride >= "
                       "nfft)", who, (unsigned long long)sym_stride, (unsigned long long)frame_stride);
    if (nframes == 0) return VIT_OK;
    LAUNCHCHK("OFDM demap launch failed: %s",
              vit_launch_ofdm_demap(d_fft, sym_stride, frame_stride, d_bins, sh, gain, nframes, d_fic, ring, col, rule, d_level,
                                    (hipStream_t)stream));
    return VIT_OK;
}

int vit_ofdm_demap_dev(const float* d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t* d_bins,
                       const vit_ofdm_shape* shape, float gain, int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring,
                       uint64_t col, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    return ofdm_demap("vit_ofdm_demap_dev", d_fft, sym_stride, frame_stride, d_bins, shape, gain, VIT_SOFT_PER_CARRIER, nframes,
                      d_fic, ring, col, nullptr, stream);
}

int vit_ofdm_demap_soft_dev(const float* d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t* d_bins,
                            const vit_ofdm_shape* shape, const vit_soft_rule* soft, int64_t nframes, uint8_t* d_fic,
                            const vit_cif_ring* ring, uint64_t col, float* d_level, void* stream) {
    const char* who = "vit_ofdm_demap_soft_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    float gain = 0.0f;
    if (ofdm_check_soft(who, soft, d_level, &gain) != VIT_OK) return VIT_ERR_ARG;
    return ofdm_demap(who, d_fft, sym_stride, frame_stride, d_bins, shape, gain, soft->rule, nframes, d_fic, ring, col, d_level,
                      stream);
}

// ---- from the samples: rotation, FFT and the demapping behind it (vit_ofdm_td.hip) --------------------------------------
int64_t vit_fft_twiddles(uint32_t nfft, float* h_tw) {
    const int64_t n = vit_fft_twiddles_host(nfft, h_tw);
    if (n < 0) set_err("vit_fft_twiddles: bad arguments (nfft=%u, a power of two 64 ... 8192)", nfft);
    return n;
}

int64_t vit_nco_table(uint32_t nco_bits, float* h_nco) {
    const int64_t n = vit_nco_table_host(nco_bits, h_nco);
    if (n < 0) set_err("vit_nco_table: bad arguments (nco_bits=%u, 1 ... 20)", nco_bits);
    return n;
}

// the rules of vit_iq_format: the float32 format of the existing calls ignores the scale
static const vit_iq_format IQ_FORMAT_F32 = {VIT_IQ_F32, 1.0f};
static int iq_check_format(const char* who, const vit_iq_format* fmt) {
    if (!fmt) return bad_arg("%s: bad arguments (NULL fmt)", who);
    if (fmt->format > VIT_IQ_CS16)
        return bad_arg("%s: bad arguments (format %u, one of VIT_IQ_F32 ... VIT_IQ_CS16)", who, fmt->format);
    if (fmt->format != VIT_IQ_F32 && !(fmt->scale >= 0x1p-32f && fmt->scale <= 0x1p16f)) {  // false for NaN
        set_err("%s: bad arguments (scale %g, 2^-32 <= scale <= 2^16)", who, (double)fmt->scale);
        return VIT_ERR_ARG;
    }
    return VIT_OK;
}
// d_iq: 8-byte aligned float32 pairs, 4-byte aligned integer samples
static int iq_check_alignment(const char* who, const void* d_iq, const vit_iq_format* fmt) {
    if (((uintptr_t)d_iq & (fmt->format == VIT_IQ_F32 ? 7u : 3u)) != 0)
        return bad_arg("%s: bad arguments (d_iq must be 8-byte aligned, 4-byte aligned for an integer format)", who);
    return VIT_OK;
}

// The tables of vit_iq_input: d_tw, d_nco and d_start (and d_rot, where the call reads one) 8-byte aligned.
static bool iq_tables_aligned(const vit_iq_input* in, bool rot) {
    return (((uintptr_t)in->d_tw | (uintptr_t)in->d_nco | (uintptr_t)in->d_start | (rot ? (uintptr_t)in->d_rot : 0)) & 7u) == 0;
}
// ... and, for the calls that read d_rot, what it needs; align_fmt is the caller's wording of the alignment rule, which
// `others` (the call's further pointers) joins
static int iq_check_tables(const char* who, const vit_iq_input* in, bool others, const char* align_fmt) {
    if (!iq_tables_aligned(in, true) || !others) return bad_arg(align_fmt, who);
    if (in->d_rot && (!in->d_nco || in->nco_bits < 1u || in->nco_bits > 20u))
        return bad_arg("%s: bad arguments (d_rot needs d_nco and nco_bits 1 ... 20, got %u)", who, in->nco_bits);
    return VIT_OK;
}

// the rules of vit_iq_input for frames of nsyms symbols of nfft samples (nfft already checked)
static int ofdm_check_input(const char* who, const vit_iq_input* in, const vit_iq_format* fmt, uint32_t nfft, uint32_t nsyms,
                            int64_t nframes) {
    if (!in || !in->d_iq || !in->d_tw || nframes < 0)
        return bad_arg("%s: bad arguments (NULL in, d_iq or d_tw, or nframes=%lld < 0)", who, (long long)nframes);
    if (iq_check_alignment(who, in->d_iq, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (iq_check_tables(who, in, true, "%s: bad arguments (d_iq, d_tw, d_nco, d_start and d_rot must be 8-byte aligned)") != VIT_OK)
        return VIT_ERR_ARG;
    // a frame's reads: start ... start + (nsyms-1)*sym_stride + nfft - 1
    const unsigned __int128 extent = (unsigned __int128)(nsyms - 1u) * in->sym_stride + nfft;
    if (in->sym_stride < nfft || extent > (unsigned __int128)UINT64_MAX)
        return bad_arg("%s: bad arguments (sym_stride %llu, >= nfft %u and a frame within 2^64 samples)", who,
                       (unsigned long long)in->sym_stride, nfft);
    if (!in->d_start && nframes > 0) {
        const unsigned __int128 end = (unsigned __int128)(uint64_t)(nframes - 1) * in->frame_stride + extent;
        if (end > (unsigned __int128)in->nsamples)
            return bad_arg("%s: bad arguments (%lld frames at frame_stride %llu read beyond nsamples %llu)", who, (long long)nframes,
                           (unsigned long long)in->frame_stride, (unsigned long long)in->nsamples);
    }
    return VIT_OK;
}

static int ofdm_fft(const char* who, const vit_iq_input* in, const vit_iq_format* fmt, uint32_t nfft, uint32_t nsyms,
                    int64_t nframes, float* d_fft, uint64_t out_sym_stride, uint64_t out_frame_stride, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!valid_nfft(nfft) || nsyms == 0)
        return bad_arg("%s: bad arguments (nfft=%u, a power of two 64 ... 8192; nsyms=%u > 0)", who, nfft, nsyms);
    if (!d_fft || ((uintptr_t)d_fft & 15u) != 0 || (out_sym_stride & 1u) != 0 || (out_frame_stride & 1u) != 0 ||
        out_sym_stride < nfft)
        return bad_arg("%s: bad arguments (d_fft must be non-NULL and 16-byte aligned, out_sym_stride %llu and out_frame_stride %llu "
                       "even, out_sym_stride >= nfft)", who, (unsigned long long)out_sym_stride, (unsigned long long)out_frame_stride);
    if (ofdm_check_input(who, in, fmt, nfft, nsyms, nframes) != VIT_OK) return VIT_ERR_ARG;
    if (nframes == 0) return VIT_OK;
    LAUNCHCHK("OFDM FFT launch failed: %s",
              vit_launch_ofdm_fft(*in, *fmt, nfft, nsyms, nframes, d_fft, out_sym_stride, out_frame_stride, (hipStream_t)stream));
    return VIT_OK;
}

int vit_ofdm_fft_dev(const vit_iq_input* in, uint32_t nfft, uint32_t nsyms, int64_t nframes, float* d_fft,
                     uint64_t out_sym_stride, uint64_t out_frame_stride, void* stream) {
    return ofdm_fft("vit_ofdm_fft_dev", in, &IQ_FORMAT_F32, nfft, nsyms, nframes, d_fft, out_sym_stride, out_frame_stride, stream);
}

int vit_ofdm_fft_iq_dev(const vit_iq_input* in, const vit_iq_format* fmt, uint32_t nfft, uint32_t nsyms, int64_t nframes,
                        float* d_fft, uint64_t out_sym_stride, uint64_t out_frame_stride, void* stream) {
    return ofdm_fft("vit_ofdm_fft_iq_dev", in, fmt, nfft, nsyms, nframes, d_fft, out_sym_stride, out_frame_stride, stream);
}

// the three demodulator entries behind their VIT_ERR_NO_DEVICE answer; rule and d_level as vit_launch_ofdm_demod takes them
static int ofdm_demod(const char* who, const vit_iq_input* in, const vit_iq_format* fmt, const uint16_t* d_bins,
                      const vit_ofdm_shape* shape, float gain, int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring,
                      uint64_t col, uint32_t rule, float* d_level, void* stream) {
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!d_bins || !shape || nframes < 0)
        return bad_arg("%s: bad arguments (NULL d_bins or shape, or nframes=%lld < 0)", who, (long long)nframes);
    if (ofdm_check_outputs(who, shape, gain, nframes, d_fic, ring, col) != VIT_OK) return VIT_ERR_ARG;
    if (ofdm_check_input(who, in, fmt, shape->nfft, shape->nsyms, nframes) != VIT_OK) return VIT_ERR_ARG;
    if (nframes == 0) return VIT_OK;
    LAUNCHCHK("OFDM demodulation launch failed: %s",
              vit_launch_ofdm_demod(*in, *fmt, d_bins, *shape, gain, nframes, d_fic, ring, col, rule, d_level, (hipStream_t)stream));
    return VIT_OK;
}

int vit_ofdm_demod_dev(const vit_iq_input* in, const uint16_t* d_bins, const vit_ofdm_shape* shape, float gain, int64_t nframes,
                       uint8_t* d_fic, const vit_cif_ring* ring, uint64_t col, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    return ofdm_demod("vit_ofdm_demod_dev", in, &IQ_FORMAT_F32, d_bins, shape, gain, nframes, d_fic, ring, col, VIT_SOFT_PER_CARRIER,
                      nullptr, stream);
}

int vit_ofdm_demod_iq_dev(const vit_iq_input* in, const vit_iq_format* fmt, const uint16_t* d_bins, const vit_ofdm_shape* shape,
                          float gain, int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring, uint64_t col, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    return ofdm_demod("vit_ofdm_demod_iq_dev", in, fmt, d_bins, shape, gain, nframes, d_fic, ring, col, VIT_SOFT_PER_CARRIER, nullptr,
                      stream);
}

int vit_ofdm_demod_soft_dev(const vit_iq_input* in, const vit_iq_format* fmt, const uint16_t* d_bins, const vit_ofdm_shape* shape,
                            const vit_soft_rule* soft, int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring, uint64_t col,
                            float* d_level, void* stream) {
    const char* who = "vit_ofdm_demod_soft_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    float gain = 0.0f;
    if (ofdm_check_soft(who, soft, d_level, &gain) != VIT_OK) return VIT_ERR_ARG;
    return ofdm_demod(who, in, fmt ? fmt : &IQ_FORMAT_F32, d_bins, shape, gain, nframes, d_fic, ring, col, soft->rule, d_level, stream);
}

// ---- from the coarse start: fine time and frequency (vit_ofdm_sync.hip) ----------------------------------------------------
static int ofdm_sync(const char* who, const vit_iq_input* in, const vit_iq_format* fmt, const vit_sync_params* p,
                     const float* d_prs, int64_t nframes, int64_t* d_start_out, uint32_t* d_rot_out, uint32_t* d_info,
                     void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!in || !p || !d_prs || !d_start_out || !d_rot_out || !in->d_iq || !in->d_tw || !in->d_nco || nframes < 0)
        return bad_arg("%s: bad arguments (NULL in, p, d_iq, d_tw, d_nco, d_prs, d_start_out or d_rot_out, or nframes=%lld < 0)", who,
                       (long long)nframes);
    if (iq_check_alignment(who, in->d_iq, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!iq_tables_aligned(in, false) || (((uintptr_t)d_prs | (uintptr_t)d_start_out | (uintptr_t)d_rot_out) & 7u) != 0 ||
        ((uintptr_t)d_info & 3u) != 0)
        return bad_arg("%s: bad arguments (d_iq, d_tw, d_nco, d_start, d_prs, d_start_out and d_rot_out must be 8-byte aligned, d_info "
                       "4-byte aligned)", who);
    if (in->d_rot || in->nco_bits < 1u || in->nco_bits > 20u)
        return bad_arg("%s: bad arguments (d_rot must be NULL - the call writes that table -, nco_bits 1 ... 20, got %u)", who,
                       in->nco_bits);
    if (!valid_nfft(p->nfft) || p->nsyms < 2u || p->cp_symbols < 1u ||
        p->cp_symbols > p->nsyms - 1u || p->M > 64u || 2u * p->M >= p->nfft || !(p->thr > 0.0f && p->thr <= 1.0f))
        return bad_arg("%s: bad arguments (nfft=%u, a power of two 64 ... 8192; nsyms=%u >= 2; cp_symbols=%u, 1 ... nsyms-1; M=%u, 0 ... "
                       "64 and 2*M < nfft; thr=%g, 0 < thr <= 1)", who, p->nfft, p->nsyms, p->cp_symbols, p->M, (double)p->thr);
    const uint64_t guard = in->sym_stride >= p->nfft ? in->sym_stride - p->nfft : 0;
    if (guard == 0 || guard > 0x7FFFFFFFull || 2ull * p->W >= guard || 2ull * p->W >= p->nfft)
        return bad_arg("%s: bad arguments (W=%u: 2*W < guard and 2*W < nfft, guard = sym_stride %llu - nfft %u, 0 < guard < 2^31)", who,
                       p->W, (unsigned long long)in->sym_stride, p->nfft);
    // a frame's reads: c - W ... c + (nsyms-1)*sym_stride + nfft - 1 + W
    const unsigned __int128 span = (unsigned __int128)(p->nsyms - 1u) * in->sym_stride + p->nfft + 2ull * p->W;
    if (span > (unsigned __int128)UINT64_MAX)
        return bad_arg("%s: bad arguments (a frame of %u symbols at sym_stride %llu spans beyond 2^64 samples)", who, p->nsyms,
                       (unsigned long long)in->sym_stride);
    if (!in->d_start && nframes > 0) {
        const __int128 first = (__int128)p->first_start - (__int128)p->W;
        const __int128 end = first + (__int128)((unsigned __int128)(uint64_t)(nframes - 1) * in->frame_stride) + (__int128)span;
        if (first < 0 || end > (__int128)in->nsamples || (unsigned __int128)(uint64_t)(nframes - 1) * in->frame_stride > (unsigned __int128)INT64_MAX)
            return bad_arg("%s: bad arguments (%lld frames from first_start %lld at frame_stride %llu read outside [0, nsamples %llu))",
                           who, (long long)nframes, (long long)p->first_start, (unsigned long long)in->frame_stride,
                           (unsigned long long)in->nsamples);
    }
    if (nframes == 0) return VIT_OK;
    LAUNCHCHK("OFDM synchronisation launch failed: %s",
              vit_launch_ofdm_sync(*in, *fmt, *p, d_prs, nframes, d_start_out, d_rot_out, d_info, (hipStream_t)stream));
    return VIT_OK;
}

int vit_ofdm_sync_dev(const vit_iq_input* in, const vit_sync_params* p, const float* d_prs, int64_t nframes,
                      int64_t* d_start_out, uint32_t* d_rot_out, uint32_t* d_info, void* stream) {
    return ofdm_sync("vit_ofdm_sync_dev", in, &IQ_FORMAT_F32, p, d_prs, nframes, d_start_out, d_rot_out, d_info, stream);
}

int vit_ofdm_sync_iq_dev(const vit_iq_input* in, const vit_iq_format* fmt, const vit_sync_params* p, const float* d_prs,
                         int64_t nframes, int64_t* d_start_out, uint32_t* d_rot_out, uint32_t* d_info, void* stream) {
    return ofdm_sync("vit_ofdm_sync_iq_dev", in, fmt, p, d_prs, nframes, d_start_out, d_rot_out, d_info, stream);
}

// ---- integer samples to the floats of the definition (vit_iq_convert.hip) ----------------------------------------------
int vit_iq_convert_dev(const void* d_iq, const vit_iq_format* fmt, uint64_t nsamples, float* d_out, void* stream) {
    const char* who = "vit_iq_convert_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (fmt->format == VIT_IQ_F32) return bad_arg("%s: bad arguments (format VIT_IQ_F32: nothing to convert)", who);
    if (!d_iq || !d_out || ((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_out & 7u) != 0 || nsamples > (UINT64_MAX >> 4))
        return bad_arg("%s: bad arguments (NULL d_iq or d_out, d_iq not 4-byte or d_out not 8-byte aligned, or nsamples=%llu >= 2^60)",
                       who, (unsigned long long)nsamples);
    if (nsamples == 0) return VIT_OK;
    LAUNCHCHK("sample conversion launch failed: %s", vit_launch_iq_convert(d_iq, *fmt, nsamples, d_out, (hipStream_t)stream));
    return VIT_OK;
}

// ---- before the stream: rate conversion and channel selection (vit_resample.hip) ---------------------------------------------
int64_t vit_resample_taps(uint32_t L, uint32_t T, double cutoff, float* h_taps) {
    if (!h_taps || L < 1u || L > 1024u || T < 4u || T > 128u || (T & 3u) != 0 || L * T > 16384u || !(cutoff > 0.0 && cutoff <= 0.5)) {
        set_err("vit_resample_taps: bad arguments (L=%u, 1 ... 1024; T=%u, a multiple of 4, 4 ... 128; L*T <= 16384; cutoff=%g, 0 < "
                "cutoff <= 0.5; h_taps non-NULL)", L, T, cutoff);
        return -1;
    }
    const double pi = 3.14159265358979323846;
    double h[128];
    for (uint32_t phi = 0; phi < L; phi++) {
        double sum = 0.0;
        for (uint32_t k = 0; k < T; k++) {
            const double u = (double)k - (double)(T / 2u - 1u) - (double)phi / (double)L;
            const double x = 2.0 * cutoff * u;
            const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
            h[k] = 2.0 * cutoff * sinc * (0.42 + 0.5 * cos(2.0 * pi * u / T) + 0.08 * cos(4.0 * pi * u / T));
            sum += h[k];
        }
        for (uint32_t k = 0; k < T; k++) h_taps[(size_t)phi * T + k] = (float)(h[k] / sum);
    }
    return (int64_t)L * T;
}

// the ranges of L, M and T: what the positions of the outputs depend on
static bool resample_ratio_ok(const vit_resample_params* p) {
    return p->L >= 1u && p->L <= 1024u && p->M >= 1u && p->M <= 4096u && p->T >= 4u && p->T <= 128u && (p->T & 3u) == 0 &&
           p->L * p->T <= 16384u;
}
static int64_t resample_out_count(uint64_t nsamples, const vit_resample_params* p) {
    if (nsamples < p->T) return 0;
    // the last output's P <= (nsamples - T + 1)*L - 1, and P stays inside 64 bits
    unsigned __int128 pmax = (unsigned __int128)(nsamples - p->T + 1u) * p->L - 1u;
    if (pmax > (unsigned __int128)UINT64_MAX) pmax = UINT64_MAX;
    if ((unsigned __int128)p->pos0 > pmax) return 0;
    const unsigned __int128 n = (pmax - p->pos0) / p->M + 1u;
    return n > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)n;
}

int64_t vit_resample_out_count(uint64_t nsamples, const vit_resample_params* p) {
    if (!p || !resample_ratio_ok(p)) {
        set_err("vit_resample_out_count: bad arguments (NULL p, or L 1 ... 1024, M 1 ... 4096, T a multiple of 4, 4 ... 128, L*T <= 16384)");
        return -1;
    }
    return resample_out_count(nsamples, p);
}

int vit_iq_resample_dev(const void* d_iq, uint64_t nsamples, const vit_iq_format* fmt, const vit_resample_params* p, int64_t nout,
                        float* d_out, uint64_t out_stride, void* stream) {
    const char* who = "vit_iq_resample_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!fmt) fmt = &IQ_FORMAT_F32;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!d_iq || !p || !p->d_taps || !d_out || nout < 0)
        return bad_arg("%s: bad arguments (NULL d_iq, p, d_taps or d_out, or nout=%lld < 0)", who, (long long)nout);
    if (iq_check_alignment(who, d_iq, fmt) != VIT_OK) return VIT_ERR_ARG;
    if ((((uintptr_t)p->d_taps | (uintptr_t)p->d_nco | (uintptr_t)d_out) & 7u) != 0)
        return bad_arg("%s: bad arguments (d_taps, d_nco and d_out must be 8-byte aligned)", who);
    if (!resample_ratio_ok(p) || p->nchan < 1u || p->nchan > VIT_RESAMPLE_MAX_CHAN || p->reserved != 0u)
        return bad_arg("%s: bad arguments (L=%u, 1 ... 1024; M=%u, 1 ... 4096; T=%u, a multiple of 4, 4 ... 128; L*T <= 16384; nchan=%u, "
                       "1 ... %u; reserved=%u, 0)", who, p->L, p->M, p->T, p->nchan, (unsigned)VIT_RESAMPLE_MAX_CHAN, p->reserved);
    if ((p->rot != nullptr) != (p->d_nco != nullptr) || (!p->rot && p->nchan > 1u) ||
        (p->rot && (p->nco_bits < 1u || p->nco_bits > 20u)))
        return bad_arg("%s: bad arguments (rot and d_nco go together, with nco_bits 1 ... 20, got %u; without them nchan=%u must be 1)",
                       who, p->nco_bits, p->nchan);
    if (nsamples > (UINT64_MAX >> 4)) return bad_arg("%s: bad arguments (nsamples=%llu >= 2^60)", who, (unsigned long long)nsamples);
    const int64_t most = resample_out_count(nsamples, p);
    if (nout > most)
        return bad_arg("%s: bad arguments (nout=%lld: %llu samples from pos0=%llu hold %lld outputs)", who, (long long)nout,
                       (unsigned long long)nsamples, (unsigned long long)p->pos0, (long long)most);
    if (p->nchan > 1u && out_stride < (uint64_t)nout)
        return bad_arg("%s: bad arguments (out_stride=%llu < nout=%lld with %u channels)", who, (unsigned long long)out_stride,
                       (long long)nout, p->nchan);
    if (nout == 0) return VIT_OK;
    LAUNCHCHK("resampler launch failed: %s", vit_launch_resample(d_iq, *fmt, *p, nout, d_out, out_stride, (hipStream_t)stream));
    return VIT_OK;
}

// ---- from the stream: first acquisition (vit_ofdm_acq.hip) ------------------------------------------------------------------
int vit_ofdm_acquire_dev(const void* d_iq, uint64_t nsamples, const vit_iq_format* fmt, const vit_acq_params* p, int64_t nperiods,
                         int64_t* d_start_out, uint32_t* d_info, float* d_power, void* stream) {
    const char* who = "vit_ofdm_acquire_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!fmt) fmt = &IQ_FORMAT_F32;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!d_iq || !p || !d_start_out || nperiods < 0)
        return bad_arg("%s: bad arguments (NULL d_iq, p or d_start_out, or nperiods=%lld < 0)", who, (long long)nperiods);
    if (iq_check_alignment(who, d_iq, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (((uintptr_t)d_start_out & 7u) != 0 || ((uintptr_t)d_info & 3u) != 0 || ((uintptr_t)d_power & 3u) != 0)
        return bad_arg("%s: bad arguments (d_start_out must be 8-byte aligned, d_info and d_power 4-byte aligned)", who);
    if (p->B < 8u || p->B > 512u || (p->B & (p->B - 1u)) != 0 || p->null_blocks < 1u || p->null_blocks > 4096u ||
        p->ref_blocks < 1u || p->ref_blocks > 4096u || p->period_blocks < 1u || !(p->thr > 0.0f && p->thr < __builtin_inff()) ||
        p->reserved != 0u)
        return bad_arg("%s: bad arguments (B=%u, a power of two 8 ... 512; null_blocks=%u and ref_blocks=%u, 1 ... 4096; period_blocks=%u "
                       ">= 1; thr=%g, finite and > 0; reserved=%u, 0)", who, p->B, p->null_blocks, p->ref_blocks, p->period_blocks,
                       (double)p->thr, p->reserved);
    if (p->first > nsamples || nsamples > (UINT64_MAX >> 4))
        return bad_arg("%s: bad arguments (first=%llu <= nsamples=%llu < 2^60)", who, (unsigned long long)p->first,
                       (unsigned long long)nsamples);
    if (nperiods == 0) return VIT_OK;
    const uint64_t nblk = (nsamples - p->first) / p->B;
    // the powers the search reads; a caller's d_power receives all of them
    const unsigned __int128 reach = (unsigned __int128)(uint64_t)nperiods * p->period_blocks + p->null_blocks + p->ref_blocks - 1u;
    const uint64_t npower = d_power || reach > (unsigned __int128)nblk ? nblk : (uint64_t)reach;
    float* power = d_power;
    ScratchLease scratch;  // without d_power the powers live in the thread's symbol scratch
    const bool leased = !d_power && npower > 0;
    if (leased) {
        const int rc = scratch.begin((size_t)npower * sizeof(float), 0, (hipStream_t)stream);
        if (rc != VIT_OK) return rc;
        power = scratch.sym<float>();
    }
    hipError_t e = vit_launch_acq_power(d_iq, *fmt, p->first, p->B, npower, power, (hipStream_t)stream);
    if (e == hipSuccess) e = vit_launch_acq_search(power, nblk, *p, nperiods, d_start_out, d_info, (hipStream_t)stream);
    LAUNCHCHK("acquisition launch failed: %s", e);
    return leased ? scratch.end() : VIT_OK;
}

// ---- transmitter identification from the null symbol (vit_ofdm_tii.hip) -------------------------------------------------------
int vit_ofdm_tii_dev(const vit_iq_input* in, const vit_iq_format* fmt, const vit_tii_params* p, const uint16_t* d_pairs,
                     int64_t nframes, uint32_t* d_tii, float* d_energy, void* stream) {
    const char* who = "vit_ofdm_tii_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (!fmt) fmt = &IQ_FORMAT_F32;
    if (iq_check_format(who, fmt) != VIT_OK) return VIT_ERR_ARG;
    if (!in || !p || !d_pairs || !d_tii || !in->d_iq || !in->d_tw || nframes < 0)
        return bad_arg("%s: bad arguments (NULL in, p, d_iq, d_tw, d_pairs or d_tii, or nframes=%lld < 0)", who, (long long)nframes);
    if (iq_check_alignment(who, in->d_iq, fmt) != VIT_OK) return VIT_ERR_ARG;
    const bool others = ((uintptr_t)d_pairs & 1u) == 0 && (((uintptr_t)d_tii | (uintptr_t)d_energy) & 3u) == 0;
    if (iq_check_tables(who, in, others, "%s: bad arguments (d_tw, d_nco, d_start and d_rot must be 8-byte aligned, d_pairs 2-byte, "
                                         "d_tii and d_energy 4-byte aligned)") != VIT_OK)
        return VIT_ERR_ARG;
    if (!valid_nfft(p->nfft) || p->ngroups < 1u || p->ngroups > 32u ||
        p->ncombs < 1u || (uint64_t)p->ngroups * p->ncombs > 1024u || p->nrep < 1u || p->nrep > 8u ||
        2ull * p->nrep * p->ngroups * p->ncombs > p->nfft || p->navg < 1u || p->navg > 256u ||
        !(p->thr > 0.0f && p->thr < __builtin_inff()))
        return bad_arg("%s: bad arguments (nfft=%u, a power of two 64 ... 8192; ngroups=%u, 1 ... 32; ncombs=%u >= 1, ngroups*ncombs <= "
                       "1024; nrep=%u, 1 ... 8, 2*nrep*ngroups*ncombs <= nfft; navg=%u, 1 ... 256; thr=%g, finite and > 0)", who,
                       p->nfft, p->ngroups, p->ncombs, p->nrep, p->navg, (double)p->thr);
    if (nframes > 0x7FFFFFFFll)
        return bad_arg("%s: bad arguments (nframes=%lld, at most 2^31 - 1 per call)", who, (long long)nframes);
    if (!in->d_start && nframes > 0) {
        // the windows t*frame_stride + offset ... + nfft - 1: the first and the last bound all of them
        const __int128 last = (__int128)((unsigned __int128)(uint64_t)(nframes - 1) * in->frame_stride);
        if (p->offset < 0 || last > (__int128)INT64_MAX || last + p->offset + p->nfft > (__int128)in->nsamples ||
            (__int128)p->offset + p->nfft > (__int128)in->nsamples)
            return bad_arg("%s: bad arguments (%lld windows of %u samples at frame_stride %llu and offset %lld read outside [0, nsamples "
                           "%llu))", who, (long long)nframes, p->nfft, (unsigned long long)in->frame_stride, (long long)p->offset,
                           (unsigned long long)in->nsamples);
    }
    if (nframes == 0) return VIT_OK;
    ScratchLease scratch;  // the frames' pair powers live in the thread's symbol scratch
    const int rc = scratch.begin((size_t)nframes * p->ngroups * p->ncombs * sizeof(float), 0, (hipStream_t)stream);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("transmitter identification launch failed: %s",
              vit_launch_ofdm_tii(*in, *fmt, *p, d_pairs, nframes, scratch.sym<float>(), d_tii, d_energy, (hipStream_t)stream));
    return scratch.end();
}

int64_t vit_tii_pair_bins(uint32_t mode, uint16_t* h_pairs) {
    if (mode != 1u || !h_pairs) {
        set_err("vit_tii_pair_bins: bad arguments (mode=%u: only mode 1 has a table; h_pairs non-NULL)", mode);
        return -1;
    }
    static const int base[4] = {-768, -384, 1, 385};
    for (int r = 0; r < 4; r++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 24; c++) {
                const int k0 = base[r] + 2 * c + 48 * b;
                h_pairs[(r * 8 + b) * 24 + c] = (uint16_t)(k0 < 0 ? 2048 + k0 : k0);
            }
    return 768;
}

int vit_tii_main_id(uint32_t mask) {
    if (mask > 255u || __builtin_popcount(mask) != 4) return -1;
    uint32_t word = 0;  // group 0 in the most significant of 8 bits
    for (uint32_t b = 0; b < 8u; b++) word |= (mask >> b & 1u) << (7u - b);
    int p = 0;
    for (uint32_t w = 0; w < word; w++) p += __builtin_popcount(w) == 4;
    return p;
}

}  // extern "C"
