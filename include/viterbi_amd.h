/*
 * viterbi_amd.h -- C ABI of libviterbi.so, the MI355X (gfx950) drop-in for the
 * compute path of Drehrumbum/viterbi.dll.
 *
 * Part 1 are the five exports of the reference's viterbi.def:4-8, same names,
 * argument meaning and return values, so a caller that binds viterbi.dll
 * (QIRX via P/Invoke, viterbi-benchmark.cpp:201-229 via GetProcAddress) binds
 * this library unchanged (SysV x86-64 instead of Win64).  Part 2 is the build's
 * own batched, device-resident extension: one 96-byte call cannot feed a GPU,
 * so the throughput path takes many frames per call.
 *
 * All entry points are thread-safe.  No entry point ever computes on the CPU:
 * when no HIP device is usable they return the error codes below.
 */
#ifndef VITERBI_AMD_H
#define VITERBI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ *
 * Part 1 -- drop-in exports (reference: viterbi.def:4-8)
 * ------------------------------------------------------------------------ */

/* Replaces `deconvolve` (deconvolve.cpp:551-554, typedef DECON viterbi.h:113;
 * caller's view viterbi-benchmark.cpp:72-73).
 *   framebits : decoded bits per frame, even, <= 9216 (deconvolve.cpp:126-127)
 *   symbols   : 4*(framebits+6) soft symbols, one per u32, low byte used
 *               (0 = strong "0", 255 = strong "1"; deconvolve.cpp:141-165)
 *   unused    : ignored, like the reference's `inputLength`
 *   decodedBits: receives (framebits+7)/8 bytes, MSB first
 * Returns 0 on success, 1 on any failure ("save mode" value of
 * viterbi_helpers.asm:184-186): bad arguments, no GPU, HIP error.
 * framebits == 0 returns 0 without touching memory (C path behaviour). */
int deconvolve(unsigned int framebits, unsigned int *symbols, int unused,
               unsigned char *decodedBits);

/* Replaces `initialize` (dllmain.cpp:156-160): clears the fault state ("save
 * mode") and makes sure the device probe has run; cheap, idempotent; returns
 * non-zero (true).  The GPU is chosen once per process, at the first call into
 * the library, from the environment variable VITERBI_AMD_DEVICE (index among the
 * gfx950 devices, default 0) -- the analogue of the reference's viterbi.txt. */
unsigned char initialize(void);

/* Replaces `RScheckSuperframe` (rschecksf.cpp:65-93).  RS(120,110) over
 * GF(2^8)/0x11D on the RSDims columns of p[120*RSDims]; corrected first 110
 * rows go to outVector[110*RSDims].  Returns the summed root counts, or -1 at
 * the first uncorrectable column; that column and all later ones are left
 * unwritten in outVector.  startIx is ignored (rschecksf.cpp:69).
 * Also -1 on bad arguments / no GPU / HIP error (see vit_last_error()). */
int RScheckSuperframe(unsigned char *p, int startIx, unsigned int RSDims,
                      unsigned char *outVector);
/* BASELINE.json spells it with a capital C; same function. */
int RSCheckSuperframe(unsigned char *p, int startIx, unsigned int RSDims,
                      unsigned char *outVector);

/* Replaces `GetCPUCaps` (viterbi_helpers.asm:48-157, bit masks
 * getcpucaps.h:27-38).  There is no x86 dispatch here: returns 0 when no
 * usable GPU was found, otherwise VIT_CAPS_GFX950 | number of CUs << 8. */
int GetCPUCaps(void);
#define VIT_CAPS_GFX950 0x1

/* Replaces `WakeUpYMM` (dllmain.cpp:54-56 / viterbi_helpers.asm:160-176): a
 * warm-up hook.  Here it creates the calling thread's HIP stream and staging
 * buffers so the first deconvolve() does not pay for them. */
void WakeUpYMM(void);

/* ------------------------------------------------------------------------ *
 * Part 2 -- batched extension (not in the reference)
 * ------------------------------------------------------------------------ */

#define VIT_OK 0
#define VIT_ERR_ARG 1
#define VIT_ERR_NO_DEVICE 2
#define VIT_ERR_HIP 3

/* Last error text of the calling thread ("" if none). */
const char *vit_last_error(void);
/* Number of usable gfx950 devices (0 = none). */
int vit_device_count(void);

/* Frame descriptor for variable-length batches.
 * sym_offset: byte offset of the frame's first soft symbol in the u8 symbol
 * buffer; MUST be a multiple of 4 (the kernels load one dword per trellis step) -
 * a descriptor that is not is skipped like one with an invalid length, its
 * output stays untouched; the frame owns 4*(framebits+6) bytes from there.
 * out_offset: byte offset of its (framebits+7)/8 output bytes. */
typedef struct vit_frame_desc {
    uint64_t sym_offset;
    uint64_t out_offset;
    uint32_t framebits; /* even, <= 9216 */
    uint32_t reserved;
} vit_frame_desc;

/* Device format of the soft symbols: one byte per symbol (the low byte of the
 * reference's u32), frames back to back: frame f at f*4*(framebits+6).
 * Decoded output: frame f at f*((framebits+7)/8), MSB first; framebits may be
 * any even number up to 9216 (a partial last byte is padded with zero bits,
 * like the reference's ChainBack writes it).
 * All *_dev calls take DEVICE pointers and enqueue on `stream` (a hipStream_t,
 * NULL = default stream) without synchronising. */
int vit_decode_batch_dev(const uint8_t *d_symbols_u8, uint8_t *d_decoded,
                         uint32_t framebits, int64_t nframes, void *stream);
/* Same, symbols still in the reference ABI format (u32 per symbol, low byte
 * used).  With a 16-byte aligned buffer the decoder
 * reads them in place (narrowing fused into the kernel); otherwise they are
 * narrowed on the device into an internal scratch buffer first. */
int vit_decode_batch_dev_u32(const uint32_t *d_symbols_u32, uint8_t *d_decoded,
                             uint32_t framebits, int64_t nframes, void *stream);
/* Variable-length batch; d_desc is a DEVICE array of nframes descriptors,
 * max_framebits the largest framebits in it (host-known).  A descriptor whose
 * framebits exceeds max_framebits (or is odd) is skipped: its output bytes stay
 * untouched.  Tables of 16 or more frames
 * are length-sorted on the device into an internal copy first (longest frame
 * first: a wavefront decodes four consecutive descriptors and runs as long as
 * the longest); d_desc itself is never modified and the order changes no
 * output byte.  Frames longer than 778 bits use a per-thread HBM scratch
 * buffer for their decision history (grown on demand). */
int vit_decode_varlen_dev(const uint8_t *d_symbols_u8, uint8_t *d_decoded,
                          const vit_frame_desc *d_desc, int64_t nframes,
                          uint32_t max_framebits, void *stream);
/* Same, for a table the caller does not trust: sym_bytes / out_bytes are the sizes of the two buffers, and a
 * descriptor whose 4*(framebits+6) symbol bytes or (framebits+7)/8 output bytes would lie (even partly) outside them
 * is skipped like the other invalid ones (checked on the device, in a copy of the table; nothing is read or written
 * for it).  vit_decode_varlen_dev itself takes no sizes: there a bad offset is an out-of-bounds device access. */
int vit_decode_varlen_dev_checked(const uint8_t *d_symbols_u8, uint64_t sym_bytes, uint8_t *d_decoded,
                                  uint64_t out_bytes, const vit_frame_desc *d_desc, int64_t nframes,
                                  uint32_t max_framebits, void *stream);
/* Host helper: reorder a HOST array of descriptors by framebits (longest first, stable) before
 * uploading it.  Optional since the device-side sort above; kept for callers that build tables of
 * fewer than 16 frames or want a deterministic order.  Every descriptor carries its own offsets,
 * so the order does not change any output byte. */
void vit_sort_descs(vit_frame_desc *h_desc, int64_t nframes);
/* u32 -> u8 narrowing of nsym symbols on the device (ingest stage). */
int vit_pack_symbols_dev(const uint32_t *d_symbols_u32, uint8_t *d_symbols_u8,
                         int64_t nsym, void *stream);

/* Host-buffer convenience: H2D, decode, D2H, synchronous. */
int vit_decode_batch_host(const uint8_t *h_symbols_u8, uint8_t *h_decoded,
                          uint32_t framebits, int64_t nframes);

/* Batched RScheckSuperframe: nsf superframes of 120*RSDims bytes each (device),
 * outputs 110*RSDims bytes each; d_ret[s] receives what RScheckSuperframe
 * would return for superframe s.  Output columns at and after the first
 * uncorrectable column of a superframe are left untouched. */
int vit_rs_batch_dev(const uint8_t *d_p, uint8_t *d_out, int32_t *d_ret,
                     uint32_t RSDims, int64_t nsf, void *stream);
int vit_rs_batch_host(const uint8_t *h_p, uint8_t *h_out, int32_t *h_ret,
                      uint32_t RSDims, int64_t nsf);

/* DAB+ superframe path: nsf superframes, each = 5 consecutive frames of
 * framebits = 192*RSDims bits in d_symbols_u8.  Decodes the 5*nsf frames into d_work
 * (nsf*120*RSDims bytes, device) -- five decoded frames ARE the RS input block p[j + k*RSDims] --
 * and runs the batched RScheckSuperframe on it.  Both kernels are enqueued on `stream`. */
int vit_dabplus_superframes_dev(const uint8_t *d_symbols_u8, uint8_t *d_work, uint8_t *d_rs_out,
                                int32_t *d_ret, uint32_t RSDims, int64_t nsf, void *stream);

/* Ingest stage for concurrent callers of deconvolve() (the reference is re-entrant and QIRX calls it from several
 * threads, README.md:56).  `microseconds` = 0 switches it off: every call is a launch of its own on its thread's stream.
 * With a window > 0, a call that finds at least `min_callers` deconvolve() calls in flight (itself included)
 * claims a slot of one mapped pinned ring, copies its own symbols into it (narrowed to one byte each) and joins the
 * open batch; the batch's first caller holds it open while `launches_in_flight` earlier batches are still on the
 * GPU - never longer than the window - and then issues ONE launch for all members; each workgroup publishes its
 * slot's completion word, on which the caller spins.  A lone caller finds a free launch credit and is launched at
 * once, so nobody waits for callers that do not exist.  No worker thread, no copy by anyone but the caller itself.
 * Environment (read when the library is loaded, for hosts that only bind the five reference exports):
 * VITERBI_AMD_BATCH_WINDOW_US, VITERBI_AMD_BATCH_MIN_CALLERS, VITERBI_AMD_BATCH_DEPTH, VITERBI_AMD_SPIN_CPUS.
 * Waiting: the batch's first caller polls the completion words; the others spin on their own word while the calls in
 * flight do not exceed `cpus` (default: the process's CPU budget - affinity mask capped by a cgroup CPU quota) and
 * otherwise sleep on a futex until the polling member wakes them (32 spinning callers in a 16-CPU container get the
 * whole process throttled).  vit_set_batch_spin_cpus(0): always sleep.
 * All setters return the previous value. */
int vit_set_batch_window_us(int microseconds);
int vit_set_batch_min_callers(int min_callers);
int vit_set_batch_depth(int launches_in_flight);
int vit_set_batch_spin_cpus(int cpus);

/* Punctured input (EN 300 401 clause 11: FIC, EEP/UEP MSC sub-channels, DAB+).  The K=7 rate-1/4 mother code's output is
 * thinned by puncturing vectors; these calls take the transmitted symbols only and write the erasures in on the device
 * before decoding.  A profile is a run of segments; segment k covers `steps` trellis steps and starts its 8-step pattern
 * period afresh at its own first step (it may end mid-period).  keep bit 4*(k mod 8) + j = symbol j of the segment's
 * k-th step is transmitted (symbol order within a step as in the u8 device format; 0 = punctured, replaced by the
 * erasure value).  A puncturing vector v0...v31 over a 32-bit sub-block is keep = sum v_i << i, i.e. 8 steps; a DAB
 * block of 128 bits is 32 steps under one vector; the 6 tail steps form a segment of their own (low 24 bits of keep).
 * A step whose four symbols are all punctured is legal.  The library compiles in no tables of the standard: the
 * caller supplies the vectors (INTEGRATION.md shows the FIC).  Transmitted symbols are one byte each, back to back in
 * step order. */
#define VIT_PUNCT_MAX_SEGS 8
typedef struct vit_punct_seg {
    uint32_t steps; /* trellis steps this segment covers (>= 1) */
    uint32_t keep;  /* period-8-step mask, see above */
} vit_punct_seg;
typedef struct vit_punct_profile {
    uint32_t nsegs; /* 1 ... VIT_PUNCT_MAX_SEGS */
    vit_punct_seg seg[VIT_PUNCT_MAX_SEGS];
} vit_punct_profile;
/* Transmitted symbols of one frame under `p`, or -1 if p is invalid or its steps do not sum to
 * framebits + 6.  Host only, needs no GPU. */
int64_t vit_punctured_length(const vit_punct_profile *p, uint32_t framebits);
/* nframes equal-length frames, frame f's transmitted symbols at f*P bytes (P = vit_punctured_length);
 * no alignment requirement on d_punct or P.  Missing symbols become `erasure`.  Decoded output as
 * vit_decode_batch_dev.  Returns VIT_ERR_ARG for an invalid profile or one that does not cover
 * framebits + 6 steps.  `profile` is a HOST pointer, read during the call.
 * The expanded symbols go to the calling thread's scratch buffer on the caller's current device (the one the u32
 * path narrows into): it grows to nframes*4*(framebits+6) bytes; its reuse across streams is ordered by an event. */
int vit_decode_punctured_dev(const uint8_t *d_punct, uint8_t *d_decoded, uint32_t framebits,
                             int64_t nframes, const vit_punct_profile *profile, uint8_t erasure,
                             void *stream);
/* Variable-length, per-frame profile: desc[i].reserved = index into the DEVICE array d_profiles
 * (nprofiles entries); sym_offset = byte offset of the frame's transmitted symbols in d_punct (any
 * alignment).  Always bounds-checked like vit_decode_varlen_dev_checked: a descriptor with odd or
 * too large framebits, a profile index >= nprofiles, an invalid profile, a profile whose steps do not
 * sum to framebits + 6, or input/output bytes outside sym_bytes/out_bytes is skipped - its output
 * bytes stay untouched.  d_desc and d_profiles are never modified.  No input byte outside a frame's own
 * [sym_offset, sym_offset + P) is read.  Scratch: frame i is expanded into slot i*4*(max_framebits+6) of the
 * thread's scratch buffer, which grows to nframes*4*(max_framebits+6) bytes, plus an internal descriptor table of
 * nframes*24 bytes; the decode then runs as vit_decode_varlen_dev on them (device sort, long-frame kernel). */
int vit_decode_punctured_varlen_dev(const uint8_t *d_punct, uint64_t sym_bytes, uint8_t *d_decoded,
                                    uint64_t out_bytes, const vit_frame_desc *d_desc, int64_t nframes,
                                    uint32_t max_framebits, const vit_punct_profile *d_profiles,
                                    uint32_t nprofiles, uint8_t erasure, void *stream);

/* After the decoder (EN 300 401 clauses 5.2.1 and 10, TS 102 563 clause 6).  Every convolutionally coded stream is
 * scrambled before encoding, so a receiver undoes the energy dispersal on the decoded bytes first, then checks them.
 * Built-in definitions:
 *   energy dispersal PRBS  p_i = p_{i-9} XOR p_{i-5}, p_{-9} ... p_{-1} all 1 (x^9 + x^5 + 1, all-ones start); it
 *                          starts 0000 0111 1011 1110 (bytes 0x07 0xBE) and has period 511.  It restarts at the first
 *                          bit of every frame (the 768-bit FIC coding block, the 24 ms logical frame of an MSC
 *                          sub-channel); decoded bit i of a frame (MSB first, the decoder's layout) is XORed with p_i;
 *                          the padding bits of a partial last byte stay as they are.
 *   FIB CRC                CRC-16, g(x) = x^16 + x^12 + x^5 + 1 (0x1021), register preset 0xFFFF, MSB first over a
 *                          FIB's bytes 0..29; bytes 30..31 hold its ones' complement, MSB first (CRC-16/GENIBUS,
 *                          check value 0xD64E).  A FIB passes when the recomputed value equals bytes 30..31.
 *   DAB+ fire code         g(x) = (x^11 + 1)(x^5 + x^3 + x^2 + x + 1) = 0x782F, register 0, no final XOR: the
 *                          remainder of a superframe's bytes 2..10 (MSB first) must equal bytes 0..1.  Checked on the
 *                          descrambled bytes before RS: the receiver's superframe-sync test.
 * Argument rules and errors as the other *_dev calls (VIT_ERR_NO_DEVICE first, VIT_ERR_ARG with vit_last_error(),
 * everything enqueued on `stream` without synchronising, an empty batch returns VIT_OK and writes nothing).  Device
 * pointers may have any alignment; no byte outside a frame's own bytes is read or written, so frames may share a
 * dword.  The decode in the chains below uses the process's renormalise comparator (vit_set_renorm_ge). */
/* Host only, needs no GPU: the PRBS as XOR bytes for one frame, (framebits+7)/8 bytes, padding bits 0.
 * Returns the byte count, or -1 for odd framebits, framebits > 9216 or a NULL h_out. */
int64_t vit_energy_dispersal_prbs(uint8_t *h_out, uint32_t framebits);
/* In place, nframes frames of (framebits+7)/8 bytes back to back (the decoded-output layout); framebits even,
 * <= 9216. */
int vit_energy_dispersal_dev(uint8_t *d_bytes, uint32_t framebits, int64_t nframes, void *stream);
/* In place, over the frames a DEVICE descriptor table names (out_offset, framebits; sym_offset and reserved are
 * ignored).  A descriptor with odd framebits, framebits > 9216, or output bytes outside [0, out_bytes) is skipped
 * (checked on the device); d_desc is not modified. */
int vit_energy_dispersal_varlen_dev(uint8_t *d_bytes, uint64_t out_bytes, const vit_frame_desc *d_desc,
                                    int64_t nframes, void *stream);
/* nfibs consecutive 32-byte FIBs (already descrambled) -> d_ok[i] = 1 if FIB i's CRC holds, else 0.  d_fibs is only
 * read. */
int vit_fib_crc_dev(const uint8_t *d_fibs, int64_t nfibs, uint8_t *d_ok, void *stream);
/* FIC chain: [depuncture ->] decode -> descramble -> FIB CRC; one kernel after the decode reads every decoded byte
 * once, writes it back descrambled and writes the flags.
 * framebits: a multiple of 256 in 256 ... 9216 (768 for the FIC coding block of modes I, II and IV).
 * profile == NULL: d_in holds depunctured u8 symbols as for vit_decode_batch_dev.
 * Otherwise: transmitted symbols as for vit_decode_punctured_dev (same scratch use).
 * d_fibs receives the descrambled frames (nframes*framebits/8 bytes), d_fib_ok nframes*framebits/256 flags. */
int vit_decode_fic_dev(const uint8_t *d_in, uint8_t *d_fibs, uint8_t *d_fib_ok, uint32_t framebits,
                       int64_t nframes, const vit_punct_profile *profile, uint8_t erasure, void *stream);
/* DAB+ chain: [depuncture ->] decode 5*nsf frames of 192*RSDims bits into d_work -> descramble each frame -> fire-code
 * flag per superframe (d_fire_ok may be NULL) -> batched RScheckSuperframe as vit_rs_batch_dev.  RSDims 1 ... 48.
 * profile NULL / non-NULL as for vit_decode_fic_dev.  (vit_dabplus_superframes_dev does not descramble: it is kept
 * for unscrambled input.) */
int vit_dabplus_punctured_superframes_dev(const uint8_t *d_in, const vit_punct_profile *profile,
                                          uint8_t erasure, uint8_t *d_work, uint8_t *d_rs_out,
                                          int32_t *d_ret, uint8_t *d_fire_ok, uint32_t RSDims,
                                          int64_t nsf, void *stream);

/* DAB+ access units (TS 102 563 clause 5.2): what the audio decoder consumes.  Built-in definition, on a superframe of
 * L = 110*RSDims bytes in natural order (the layout of d_rs_out), RSDims 1 ... 48:
 *   bytes 0..1             the fire code over bytes 2..10, as above
 *   byte 2                 bit 7 rfa, bit 6 dac_rate, bit 5 sbr_flag, bit 4 aac_channel_mode, bit 3 ps_flag,
 *                          bits 2..0 mpeg_surround_config
 *   num_aus                from (dac_rate, sbr_flag): (0,1) -> 2, (1,1) -> 3, (0,0) -> 4, (1,0) -> 6
 *   au_start[0]            the header's length: 5, 6, 8 or 11 bytes for num_aus 2, 3, 4 or 6
 *   au_start[1..num_aus-1] 12-bit big-endian fields packed from byte 3 on (four padding bits follow when num_aus is 2
 *                          or 4): au_start[1] = b3<<4 | b4>>4, au_start[2] = (b4&15)<<8 | b5,
 *                          au_start[3] = b6<<4 | b7>>4, au_start[4] = (b7&15)<<8 | b8, au_start[5] = b9<<4 | b10>>4
 *   au_start[num_aus]      L
 *   header validity        the library's rule: au_start[n+1] - au_start[n] >= 3 for every n in 0 ... num_aus-1, that is
 *                          strictly increasing, inside the superframe, and at least one byte in front of each CRC
 *   AU n                   bytes au_start[n] ... au_start[n+1]-1; its last two bytes hold the ones' complement of the
 *                          CRC-16 of the FIB check (0x1021, preset 0xFFFF, MSB first) over all the bytes before them
 * Example: byte 2 = 0x00 and bytes 3..7 = 12 34 56 78 90 give 4 AUs starting at 8, 0x123, 0x456 and 0x789. */
#define VIT_AU_OK 0          /* header parsed and valid; crc_ok is meaningful */
#define VIT_AU_RS_FAILED 1   /* d_ret[s] < 0: superframe not read, every other field 0 */
#define VIT_AU_BAD_HEADER 2  /* au_start rule violated: num_aus, param, fire_ok and au_start as parsed, crc_ok 0 */
typedef struct vit_au_table {   /* 20 bytes, one per superframe */
    uint8_t  status, num_aus, param /* byte 2 */, crc_ok /* bit n: AU n's CRC holds */;
    uint16_t au_start[7];       /* [0 .. num_aus]; unused entries 0 */
    uint8_t  fire_ok, reserved; /* fire code recomputed on the bytes given (after RS: on the corrected ones) */
} vit_au_table;
/* Superframe s lies at d_sf + s*sf_stride, sf_stride >= 110*RSDims; base pointer and stride may have any alignment,
 * d_au must be 4-byte aligned.  d_sf is only read, and no byte outside a superframe's own L bytes is read; every record
 * is written completely (reserved = 0).  d_ret (may be NULL) is the RS return value per superframe: a negative one gives
 * VIT_AU_RS_FAILED.  sf_stride = 110*RSDims reads d_rs_out of the DAB+ chains (on the same stream, after the chain
 * call); sf_stride = 120*RSDims with d_ret = NULL reads the first 110 rows of d_work, the superframe before RS, whose
 * AUs with a good CRC are usable even where RS gave up on a column.  One wavefront per superframe; errors as above. */
int vit_dabplus_aus_dev(const uint8_t *d_sf, uint64_t sf_stride, uint32_t RSDims, int64_t nsf,
                        const int32_t *d_ret, vit_au_table *d_au, void *stream);
/* Host only, needs no GPU: the same definition for one superframe (no RS gating).  VIT_ERR_ARG for a NULL pointer or
 * RSDims outside 1 ... 48. */
int vit_dabplus_aus_host(const uint8_t *h_sf, uint32_t RSDims, vit_au_table *h_out);
/* d_ok[i] = 1 if bytes 0..1 at d_bytes + i*stride equal the fire remainder of bytes 2..10 there, else 0 (n candidates,
 * 11 bytes read of each, any alignment).  With stride = 24*RSDims over descrambled decoded frames (d_work) every logical
 * frame is tested as a superframe start in one call. */
int vit_fire_code_dev(const uint8_t *d_bytes, uint64_t stride, int64_t n, uint8_t *d_ok, void *stream);

/* From the CIF stream: MSC time de-interleaving (EN 300 401 clause 12).  Every MSC sub-channel (DAB and DAB+ audio,
 * data; not the FIC) is spread over 16 logical frames, so a CIF carries one sixteenth of each of 16 logical frames.
 * Built-in definition:
 *   F = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15}     (F[k] = k with its 4 bits reversed)
 *   transmitter:  bit i of a sub-channel in CIF r  =  bit i of its logical frame r - F[i mod 16]
 *   these calls:  byte i of logical frame n of the call  =  ring row (first_row + n + F[i mod 16]) mod nrows,
 *                 column col + i
 * i counts the sub-channel's transmitted (punctured) symbols from its first one, one soft byte per symbol - the order
 * vit_decode_punctured_dev reads.  Frame n needs rows n ... n+15 and is complete once they are in, so a receiver's first
 * call may start at the row of the first CIF it received.  Only the 15 logical frames before that one, whose bytes began
 * in CIFs it never received, are incomplete, and no call addresses them.
 * Whole MSC at once: sub-channels start at whole CUs of 64 bits and 64 = 0 (mod 16), so in a row that starts at CU 0
 * a sub-channel's i mod 16 equals its column mod 16.  One de-interleave over the whole MSC width (col = the row's
 * CU 0) therefore de-interleaves every sub-channel at once; a sub-channel then starts at column 64*startCU of each
 * de-interleaved frame.  (A start that is not a multiple of 16 columns breaks this.)
 * The input is a ring of CIF rows on the device, so a streaming receiver never copies the 15-row overlap between
 * calls.  The struct is a HOST struct, read during the call.
 * Argument rules as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL
 * ring or d_base, first_row >= nrows, nframes + 15 > nrows (the call's rows must be distinct ring rows),
 * col + ncols > row_bytes, or an invalid profile; an empty batch returns VIT_OK and writes nothing; everything is
 * enqueued on `stream` without synchronising.
 * Guarantees: the call reads no byte outside columns [col, col + ncols) of its nframes + 15 rows, so the front end may
 * be writing other rows of the ring meanwhile (ordering between the two is the caller's, with streams and events).
 * Pointers, col and row_bytes may have any alignment. */
typedef struct vit_cif_ring {
    const uint8_t *d_base;  /* device; row r at d_base + r * row_bytes */
    uint64_t row_bytes;     /* row stride: one CIF in the caller's layout */
    uint32_t nrows;         /* rows in the ring */
    uint32_t first_row;     /* < nrows: the row of the call's frame 0 (its F = 0 bytes) */
} vit_cif_ring;
/* Frame n's ncols de-interleaved bytes to d_out + n*ncols (nothing else is written).  The whole-CIF recipe: one call
 * over the whole MSC width, then vit_decode_punctured_varlen_dev with sym_offset = n*ncols + 64*startCU per
 * sub-channel frame. */
int vit_time_deinterleave_dev(const vit_cif_ring *ring, uint64_t col, uint32_t ncols, uint8_t *d_out,
                              int64_t nframes, void *stream);
/* One sub-channel, columns [col, col + P) with P = vit_punctured_length(profile, framebits), decoded over nframes
 * consecutive logical frames; the de-interleave is fused into the depuncturing expansion.  Output and scratch use as
 * vit_decode_punctured_dev; `profile` is required. */
int vit_decode_punctured_ti_dev(const vit_cif_ring *ring, uint64_t col, uint8_t *d_decoded, uint32_t framebits,
                                int64_t nframes, const vit_punct_profile *profile, uint8_t erasure, void *stream);
/* The DAB+ chain of vit_dabplus_punctured_superframes_dev from the ring: 5*nsf logical frames (5*nsf + 15 rows).
 * `profile` is required (no NULL form). */
int vit_dabplus_ti_superframes_dev(const vit_cif_ring *ring, uint64_t col, const vit_punct_profile *profile,
                                   uint8_t erasure, uint8_t *d_work, uint8_t *d_rs_out, int32_t *d_ret,
                                   uint8_t *d_fire_ok, uint32_t RSDims, int64_t nsf, void *stream);

/* A whole ensemble: every sub-channel of the MSC in one table-driven chain.  The calls above take one sub-channel; a
 * multiplex carries a dozen or more DAB+ services of different sizes whose superframes start at different CIF phases,
 * and often a data or DAB audio sub-channel beside them.  The table below names them all, and each call here is a
 * fixed number of launches whatever the table's length.
 * The table is a HOST array, read during the call like `profile` of the uniform calls (it travels in the kernel
 * arguments; nothing is uploaded).  Entry k:
 *   DAB+ (RSDims 1 ... 48)   nframes/5 superframes of five logical frames of framebits = 192*RSDims bits; decoded,
 *                            descrambled, fire code, RS, access units
 *   not DAB+ (RSDims 0)      nframes logical frames of framebits bits (a multiple of 8): decoded and descrambled only
 * Layout rule (vit_ensemble_layout computes it; it is fixed):
 *   - sub-channels come in table order;
 *   - in d_work, sub-channel k's decoded and descrambled frames lie back to back at framebits/8 bytes each from
 *     work_offset[k] (DAB+: five frames are one RS input block of 120*RSDims bytes, as in the chains above);
 *   - in d_rs_out, its superframes lie back to back at 110*RSDims bytes each from rs_offset[k]; a sub-channel that is
 *     not DAB+ takes nothing there;
 *   - every sub-channel's block starts at the next multiple of 16 bytes behind the previous one's end (the first at 0);
 *     work_bytes / rs_bytes are the end of the last block;
 *   - d_ret, d_fire_ok and d_au hold one record per superframe in table order, DAB+ sub-channels only: sub-channel k's
 *     superframe s is record rec_index[k] + s (rec_index of an entry that is not DAB+ is the next DAB+ entry's).
 * vit_ensemble_layout needs no GPU.  It returns VIT_ERR_ARG, with vit_last_error() naming the entry, for nsub outside
 * 1 ... VIT_ENS_MAX_SUBCH, a framebits that is 0, above 9216 or no multiple of 8, RSDims > 48, a DAB+ entry whose
 * framebits is not 192*RSDims or whose nframes is no multiple of 5, nframes = 0, phase + nframes + 15 beyond 32 bits,
 * or a non-zero reserved field.  Every device entry point below runs the same validation first. */
#define VIT_ENS_MAX_SUBCH 64
typedef struct vit_ens_subch {   /* 32 bytes */
    uint32_t col;        /* column of its first transmitted symbol, relative to msc_col (64 * start CU) */
    uint32_t profile;    /* index into d_profiles */
    uint32_t framebits;  /* per logical frame: a multiple of 8, 8 ... 9216; DAB+: exactly 192*RSDims */
    uint32_t RSDims;     /* 0: not DAB+ (decode + descramble only); 1 ... 48: DAB+ */
    uint32_t phase;      /* logical frame of the call at which this sub-channel starts (DAB+: a superframe start) */
    uint32_t nframes;    /* logical frames to process, >= 1; DAB+: a multiple of 5 */
    uint32_t nsym;       /* transmitted symbols per frame = vit_punctured_length(its profile, framebits) */
    uint32_t reserved;   /* 0 */
} vit_ens_subch;
typedef struct vit_ens_layout {
    uint64_t work_offset[VIT_ENS_MAX_SUBCH], rs_offset[VIT_ENS_MAX_SUBCH], rec_index[VIT_ENS_MAX_SUBCH];
    uint64_t work_bytes, rs_bytes, nrec;    /* sizes of d_work, d_rs_out; records in d_ret / d_fire_ok / d_au */
    uint32_t rows_needed, max_framebits;    /* max(phase + nframes) + 15; largest framebits */
} vit_ens_layout;
int vit_ensemble_layout(const vit_ens_subch *h_sub, uint32_t nsub, vit_ens_layout *h_out);
/* Table forms of the stages after the decoder, ONE launch each over all DAB+ sub-channels of the table (entries that
 * are not DAB+ are passed over; col, profile, phase and nsym are not used).  Per superframe the result is what
 * vit_rs_batch_dev / vit_dabplus_aus_dev give for that sub-channel alone on the same bytes: the first-failure rule
 * (columns at and after the first uncorrectable one stay untouched), the return value, VIT_AU_RS_FAILED gating and
 * every byte of the record.  Bytes of d_rs_out between the sub-channels' blocks are never written.
 * vit_rs_table_dev: d_work / d_rs_out in the layout above, d_ret[rec_index[k] + s].
 * vit_dabplus_aus_table_dev: from_work = 0 reads d_sf in the layout of d_rs_out; from_work = 1 reads it in the layout of
 * d_work, the first 110 rows of every superframe before RS (with d_ret = NULL: the salvage pass, see
 * vit_dabplus_aus_dev).  d_au must be 4-byte aligned. */
int vit_rs_table_dev(const uint8_t *d_work, uint8_t *d_rs_out, int32_t *d_ret,
                     const vit_ens_subch *h_sub, uint32_t nsub, void *stream);
int vit_dabplus_aus_table_dev(const uint8_t *d_sf, int from_work, const vit_ens_subch *h_sub, uint32_t nsub,
                              const int32_t *d_ret /* may be NULL */, vit_au_table *d_au, void *stream);
/* The chain.  For sub-channel k with layout offsets (wo, ro, ri), take ring_k = ring with first_row advanced by phase
 * modulo nrows.  DAB+: byte for byte what
 *   vit_dabplus_ti_superframes_dev(&ring_k, msc_col + col, &profile, erasure, d_work + wo, d_rs_out + ro, d_ret + ri,
 *                                  d_fire_ok + ri, RSDims, nframes/5, stream);
 *   vit_dabplus_aus_dev(d_rs_out + ro, 110*RSDims, RSDims, nframes/5, d_ret + ri, d_au + ri, stream);
 * write; not DAB+: what vit_decode_punctured_ti_dev into d_work + wo followed by vit_energy_dispersal_dev writes.
 * d_fire_ok and d_au may be NULL (that stage's output is not produced).
 * Checked on the host before anything is launched (VIT_ERR_ARG): the table as above; the ring as for the *_ti_dev
 * calls, with rows_needed distinct rows; every sub-channel's columns [msc_col + col, + nsym) inside a row; col a
 * multiple of 16 (sub-channels start at whole CUs; see "Whole MSC at once" above); profile < nprofiles; the pointers.
 * d_profiles is a DEVICE array, so the profiles' contents are checked on the device, per frame, as
 * vit_decode_punctured_varlen_dev does: a frame whose profile is invalid, or whose steps do not sum to framebits + 6,
 * or which would read beyond its row's span, is skipped - its d_work bytes stay as they were, descrambling included -
 * and the later stages (fire code, RS, access units) see what d_work held.  vit_punctured_length is the host-side
 * check of a profile; nsym must be its value (a wrong nsym decodes the wrong columns of the call's own span, never
 * memory outside it).
 * Launches: one time de-interleave over the span of columns the table uses, the descriptor table written on the
 * device from the sub-channel table, the expansion, the decode (device sort and long-frame kernel as
 * vit_decode_varlen_dev), one descramble + fire code pass, vit_rs_table_dev, vit_dabplus_aus_table_dev.  Scratch (the
 * calling thread's, as above): (rows_needed - 15) * span bytes, 4*(max_framebits+6) bytes per frame of the table and
 * two descriptor tables of 24 bytes per frame. */
int vit_ensemble_dev(const vit_cif_ring *ring, uint64_t msc_col, const vit_ens_subch *h_sub, uint32_t nsub,
                     const vit_punct_profile *d_profiles, uint32_t nprofiles, uint8_t erasure,
                     uint8_t *d_work, uint8_t *d_rs_out, int32_t *d_ret, uint8_t *d_fire_ok /* may be NULL */,
                     vit_au_table *d_au /* may be NULL */, void *stream);

/* Packet mode (EN 300 401 clause 5.3): data sub-channels - the third kind beside DAB+ and DAB audio - and the forward
 * error correction of enhanced packet mode.  The definitions below are the library's, written without the standard's
 * text at hand; they are what these calls promise and what the tests check.  Each constant stands once in
 * csrc/vit_packet_fmt.h.
 * The stream: a packet-mode sub-channel's descrambled logical frames back to back, framebytes each, a multiple of 24 in
 * 24 ... 1152 - the d_work block of an RSDims 0 entry of vit_ensemble_dev from work_offset[k] on, or the output of the
 * decode calls after vit_energy_dispersal_dev.  It is a run of 24-byte slots, slot i = bytes 24i ... 24i+23.
 * Common rules: errors as above (VIT_ERR_NO_DEVICE first, VIT_ERR_ARG with vit_last_error()); everything is enqueued on
 * `stream` without synchronising; an empty batch (nslots or nframes 0) returns VIT_OK and writes nothing; byte pointers
 * may have any alignment, record and score pointers must be 4-byte aligned; no byte outside the named ranges is read or
 * written.
 *
 * A packet: 1 ... 4 slots.
 *   byte 0   bits 7..6 length (0 ... 3: 24, 48, 72, 96 bytes), bits 5..4 continuity index, bits 3..2 first/last,
 *            bits 1..0 address bits 9..8
 *   byte 1   address bits 7..0; address 0 is padding, address 1022 an FEC packet (always one slot)
 *   byte 2   bit 7 command, bits 6..0 useful data length
 *   last two bytes: the ones' complement of the CRC-16 of the FIB check (0x1021, preset 0xFFFF, MSB first) over all the
 *            bytes before them
 * An FEC frame: 103 slots = 94 slots of application data (2256 bytes), then 9 FEC packets.  FEC packet c (0 ... 8) has
 * byte 0 = c<<2 | 3 and byte 1 = 0xFE (length 0, a 4-bit counter in bits 5..2, address 1022), then 22 parity bytes.
 *   table    12 rows of 188 data columns, filled column by column: row r, column c = frame byte 12c + r
 *   parity   16 bytes per row; parity byte j of row r is RS-data byte m = 12j + r, at byte 2 + m % 22 of FEC packet
 *            m / 22; the last 6 bytes of FEC packet 8 are padding.  Padding and the nine headers are never changed.
 *   code     each row of 204 bytes is a codeword of RS(204,188) over GF(2^8), field polynomial 0x11D, alpha = 2,
 *            g(x) = prod_{i=0..15} (x + alpha^i), shortened from (255,239) by 51 leading zero bytes; column 0 is the
 *            highest-degree coefficient, parity byte 15 the constant term
 *   result   if a codeword of the shortened code lies within Hamming distance 8 of the row's 204 bytes (it is then the
 *            only one), every byte that differs is replaced by the codeword's, parity included, and nerr[r] is the
 *            distance (0 ... 8); otherwise the row stays as it was and nerr[r] = -1.  A nearest full-length codeword that
 *            differs in the 51 padding positions is such a failure, not a correction. */
typedef struct vit_fec_rec {   /* 16 bytes per FEC frame, written completely */
    int8_t   nerr[12];
    uint16_t hdr_ok;           /* bit c: FEC packet c's two header bytes are as expected (decoding does not depend on it) */
    uint8_t  status;           /* 0: all rows decoded; 1: at least one row failed */
    uint8_t  reserved;         /* 0 */
} vit_fec_rec;
#define VIT_PKT_CONT    0   /* slot inside a longer packet; every other field 0 */
#define VIT_PKT_DATA    1   /* a packet starts here; address not 0 and not 1022 */
#define VIT_PKT_PADDING 2   /* address 0; CRC still checked, the other fields as for a data packet */
#define VIT_PKT_FEC     3   /* address 1022: one slot whatever its length bits say, no CRC (crc_ok 0), nslots 1,
                               flags = the 4-bit counter (byte 0 bits 5..2), useful 0 */
#define VIT_PKT_OVERRUN 4   /* the length claimed here runs past the frame's end: this slot and every later slot of the
                               frame, other fields 0 */
typedef struct vit_packet_rec {   /* 8 bytes per slot, written completely */
    uint8_t  kind, crc_ok, nslots /* 1..4 at a start */, flags /* bits 1..0 continuity, 3..2 first/last, 4 command */;
    uint16_t address;
    uint8_t  useful, reserved;
} vit_packet_rec;
/* Where the FEC frames lie: d_score[p], p = 0 ... 102, = the number of slots i < nslots with (i - p) mod 103 >= 94 whose
 * first two bytes are the header of FEC packet (i - p) mod 103 - 94.  The caller takes the phase from the largest score
 * (the analogue of vit_fire_code_dev).  All 103 words are written (cleared on the stream, then added to).  d_stream is
 * only read, two bytes of each slot. */
int vit_packet_fec_sync_dev(const uint8_t *d_stream, int64_t nslots, uint32_t *d_score /* uint32[103] */, void *stream);
/* Whole FEC frames in nslots slots from `phase` on: (nslots - phase) / 103, 0 if nslots <= phase; -1 for nslots < 0 or
 * phase > 102.  Host only. */
int64_t vit_packet_fec_count(int64_t nslots, uint32_t phase);
/* phase 0 ... 102: FEC frame k occupies slots phase + 103k ... phase + 103k + 102; the nfec = vit_packet_fec_count(nslots,
 * phase) whole frames are decoded (a partial frame at the end is not), one record each.  d_out is d_stream itself (in
 * place) or does not overlap it; out of place every one of the 24*nslots bytes that is not rewritten is copied, also
 * when nfec is 0.  d_fec may be NULL when nfec is 0.  A lane per (frame, row), 20 frames per workgroup; in place, a
 * workgroup whose rows are all clean writes no byte of the stream.  Across calls the phase is the caller's:
 * (phase - slots consumed) mod 103. */
int vit_packet_fec_dev(const uint8_t *d_stream, uint8_t *d_out, int64_t nslots, uint32_t phase,
                       vit_fec_rec *d_fec /* vit_fec_rec[nfec] */, void *stream);
/* Host only, needs no GPU: the same definition for one FEC frame of 2472 bytes, in place.  VIT_ERR_ARG for a NULL
 * pointer. */
int vit_packet_fec_frame_host(uint8_t *frame /* uint8_t[2472] */, vit_fec_rec *out);
/* One record per slot of nframes logical frames of framebytes bytes at d_bytes (only read).  Per frame the walk starts
 * at slot 0: a packet starts there, its length field says where the next one starts, and so on; the walk trusts the
 * length field whether or not the CRC holds and starts again at the next frame.  One wavefront per 64 / (framebytes/24)
 * logical frames, a lane per slot. */
int vit_packets_dev(const uint8_t *d_bytes, uint32_t framebytes, int64_t nframes,
                    vit_packet_rec *d_rec /* vit_packet_rec[nframes*framebytes/24] */, void *stream);
/* MSC data groups (clause 5.3.3) from the packets: what Slideshow, TPEG, EPG and Journaline decoders consume.  Like the
 * rest of packet mode these definitions are the library's, written without the standard's text at hand; they are what
 * these calls promise and what the tests check.
 * Input: the stream d_bytes, 24*nslots bytes at any alignment, and d_rec, the nslots records that vit_packets_dev wrote
 * for it (4-byte aligned); both are only read.  Logical frames no longer matter: the records carry what they decided.
 * 1 <= nslots <= 1<<24; nslots == 0 returns VIT_OK and writes nothing.
 * Usable packets: slot i is a usable packet if kind == VIT_PKT_DATA, crc_ok == 1 and useful <= 24*nslots_i - 5.  A
 *   VIT_PKT_DATA slot that fails one of the last two is unusable.  Unusable packets and every other kind take no further
 *   part.  (Records that vit_packets_dev did not write for this window could claim a packet that ends behind the window's
 *   last slot or an address above 1023: such a slot is unusable as well, so that no byte outside the stream is read.)  A usable packet's data is bytes 3 ... 3+useful-1 of the packet, its continuity index flags & 3, and it is a
 *   first / last packet by the bits VIT_PKT_FIRST / VIT_PKT_LAST of flags.
 * Runs: per address, the usable packets in slot order.  Packet q continues its predecessor p of the same address iff q
 *   has no first flag, p has no last flag and cont(q) == (cont(p)+1) & 3.  A run is a maximal sequence in which each
 *   packet continues the one before.
 * A run is a data group iff its head has the first flag and its tail the last flag (one packet with both is a group).
 *   It is open iff its head has the first flag, its tail has no last flag and its tail is the address's last usable
 *   packet of the window.  The packets of every other run are dropped.  (The walk per address - open at a first flag,
 *   break on a wrong continuity index or a new first flag, close at a last flag - stated free of any order of evaluation.)
 * Order and layout: groups are numbered k = 0, 1, ... by ascending slot of their last packet.  Group k's bytes D[0..L) are
 *   the data of its packets in slot order; offset_0 = 0, offset_(k+1) = offset_k + L_k rounded up to a multiple of 16.
 * Header of a group: L < 2 is malformed.  b0 = D[0]: ext b0>>7, crcf (b0>>6)&1, seg (b0>>5)&1, ua (b0>>4)&1, type b0&15.
 *   cont_rep = D[1] (continuity index in the high nibble, repetition index in the low).  p = 2, then in this order: if ext,
 *   p += 2; if seg, segment = D[p]<<8 | D[p+1] (bit 15: last segment), p += 2; if ua, li = D[p]&15, tidf = (D[p]>>4)&1,
 *   p += 1, a tidf with li < 2 is malformed, a tidf with li >= 2 gives transport_id = D[p]<<8 | D[p+1], then p += li.
 *   payload_offset = p.  The header is well-formed iff every byte named lies before E = L - (crcf ? 2 : 0) and p <= E.
 *   A malformed group has flags, segment, transport_id and payload_offset 0 (crc_ok with them) and keeps type and
 *   cont_rep (0 too if L < 2).  If crcf and well-formed, crc_ok is set when the CRC-16 of D[0..L-2) - 0x1021, preset
 *   0xFFFF, complemented: the packets' own - equals D[L-2]<<8 | D[L-1]. */
#define VIT_PKT_LAST  4   /* vit_packet_rec.flags bit 2 */
#define VIT_PKT_FIRST 8   /* vit_packet_rec.flags bit 3 */
typedef struct vit_dgroup_rec {      /* 32 bytes per data group, written completely */
    uint32_t first_slot, last_slot, npackets, offset, length;
    uint16_t address, segment, transport_id, payload_offset;
    uint8_t  type, cont_rep,
             flags,     /* bit 0 well-formed, 1 crcf, 2 crc_ok, 3 seg, 4 ua, 5 tidf, 6 ext */
             command;   /* the command bit of the first packet */
} vit_dgroup_rec;
typedef struct vit_dgroup_summary {  /* 32 bytes, written completely by every call with nslots > 0 */
    uint32_t ngroups;      /* data groups found */
    uint32_t nwritten;     /* records written: a prefix */
    uint32_t data_bytes;   /* offset_ngroups: what d_data must hold for all of them */
    uint32_t open_from;    /* the smallest first slot of an open run; nslots if there is none */
    uint32_t n_used, n_dropped, n_unusable;   /* packets: in groups, dropped, unusable */
    uint32_t reserved;     /* 0 */
} vit_dgroup_summary;
/* Group k is written - its record to d_dg[k], its bytes to d_data + offset_k - iff k < max_groups and either d_data is
 * NULL or offset_k + L_k <= data_capacity; offsets grow, so the written groups are a prefix.  With d_data NULL nothing
 * is gathered, but header and CRC fields are still computed from the stream (records only).  Bytes of d_data outside
 * [offset_k, offset_k + L_k) of written groups and records >= nwritten are never written; no byte outside the named
 * ranges is read.  Enqueued on `stream` without synchronising; the result does not depend on scheduling: two runs give
 * the same bytes.
 * Across calls: the call is stateless.  open_from says where the next window must begin for no group to be lost (a
 * group that was open closes in a window that holds its first packet); groups the caller has seen already come again
 * in such a window and are recognised by their slots.
 * Errors: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG with vit_last_error() for nslots outside 0 ... 1<<24 and, with nslots > 0,
 * for a NULL d_bytes, d_rec or d_sum, a NULL d_dg with max_groups > 0, a d_rec, d_dg or d_sum that is not 4-byte
 * aligned, or a NULL d_data with data_capacity > 0.
 * Launches: which addresses have usable packets; a workgroup per such address and chunk of 16384 slots, twice (the state a
 * chunk hands on, then every closing packet's run); three of a prefix sum over the slots (numbers, offsets, summary); a
 * wavefront per written group (gather, CRC, header).  Scratch (the calling thread's): 16 bytes per slot, 16 per address
 * and chunk, 32 per 4096 slots. */
int vit_data_groups_dev(const uint8_t *d_bytes, const vit_packet_rec *d_rec, int64_t nslots,
                        vit_dgroup_rec *d_dg, uint32_t max_groups, vit_dgroup_summary *d_sum,
                        uint8_t *d_data /* may be NULL */, uint32_t data_capacity, void *stream);
/* Host only, needs no GPU: the same definition on host memory (no alignment rule; otherwise the same VIT_ERR_ARG). */
int vit_data_groups_host(const uint8_t *bytes, const vit_packet_rec *rec, int64_t nslots,
                         vit_dgroup_rec *dg, uint32_t max_groups, vit_dgroup_summary *sum,
                         uint8_t *data /* may be NULL */, uint32_t data_capacity);
/* Packet mode for a whole ensemble: up to 64 streams in one call - for each the FEC phase found on the device, RS(204,188)
 * in place and the packet records - in a number of launches that does not depend on the table's length, and without the
 * host waiting between the stages (the per-stream recipe takes the phase from the scores on the host).  The streams lie in
 * one allocation, typically d_work of vit_ensemble_dev with offset = work_offset[k] of the RSDims 0 entries that FIG 0/2
 * says are packet mode (the caller's decision).
 * Layout (vit_packet_table_layout): streams in table order; nslots_k = nframes * framebytes / 24; rec_index is the running
 * sum of nslots_k; stream k reserves nslots_k / 103 FEC records from fec_index[k] - the count at phase 0, the largest any
 * phase gives, and for every stream whatever its fec mode - so that d_fec is sized before the device has chosen a
 * phase.  Only the first nfec of a stream's FEC records are written; the others keep their bytes.
 * VIT_ERR_ARG, with vit_last_error() naming the entry, for nstreams outside 1 ... 64, a framebytes that is not a multiple
 * of 24 in 24 ... 1152, nframes 0, fec > 2, phase > 102, a non-zero phase or min_score where the mode does not use it, a
 * non-zero reserved, two streams whose byte ranges overlap, or more than 2^31 slots in the table. */
#define VIT_PKT_MAX_STREAMS 64          /* = VIT_ENS_MAX_SUBCH */
#define VIT_PKT_FEC_NONE   0            /* plain packet mode: no FEC stage, stream untouched */
#define VIT_PKT_FEC_PHASE  1            /* enhanced packet mode, phase given in the entry */
#define VIT_PKT_FEC_SEARCH 2            /* enhanced packet mode, phase found on the device */
#define VIT_PKT_NO_PHASE 0xFFFFFFFFu
typedef struct vit_pkt_stream {         /* 32 bytes, host table entry */
    uint64_t offset;                    /* bytes from d_bytes to the stream's first byte; any alignment */
    uint32_t framebytes;                /* a multiple of 24 in 24 ... 1152 */
    uint32_t nframes;                   /* logical frames, >= 1 */
    uint32_t fec;                       /* VIT_PKT_FEC_* */
    uint32_t phase;                     /* FEC_PHASE: 0 ... 102; otherwise 0 */
    uint32_t min_score;                 /* FEC_SEARCH: a phase is accepted iff its score >= max(min_score, 1); otherwise 0 */
    uint32_t reserved;                  /* 0 */
} vit_pkt_stream;
typedef struct vit_pkt_layout {
    uint64_t rec_index[VIT_PKT_MAX_STREAMS];   /* first vit_packet_rec of stream k (slots of earlier streams) */
    uint64_t fec_index[VIT_PKT_MAX_STREAMS];   /* first vit_fec_rec of stream k */
    uint64_t nrec, nfecrec;                    /* sizes of d_rec, d_fec in records */
    uint64_t bytes_end;                        /* max(offset + 24*nslots): what d_bytes must hold */
} vit_pkt_layout;
typedef struct vit_pkt_stream_rec {     /* 16 bytes per stream, written completely */
    uint32_t phase;                     /* the phase used, or VIT_PKT_NO_PHASE (FEC_NONE, or no score reached min_score) */
    uint32_t score, runner_up;          /* FEC_SEARCH: largest score and the largest score at any OTHER phase; otherwise 0 */
    uint32_t nfec;                      /* FEC frames decoded = vit_packet_fec_count(nslots, phase), 0 without a phase */
} vit_pkt_stream_rec;
/* Host only, needs no GPU. */
int vit_packet_table_layout(const vit_pkt_stream *h_tab, uint32_t nstreams, vit_pkt_layout *h_out);
/* For stream k, with s = d_bytes + offset and nslots = nslots_k, byte for byte what the per-stream calls write:
 *   FEC_SEARCH   the scores are those of vit_packet_fec_sync_dev(s, nslots, .); score is the largest of the 103, phase
 *                the SMALLEST p that has it, runner_up the largest score at any other p.  If score < max(min_score, 1)
 *                the stream has no phase: VIT_PKT_NO_PHASE, nfec 0, no byte of the stream changed.
 *   with a phase (given or found): the stream and the records are those of vit_packet_fec_dev(s, s, nslots, phase,
 *                d_fec + fec_index[k]) - always in place; a workgroup of clean rows writes no byte of the stream.
 *   then, for every stream, the records of vit_packets_dev(s, framebytes, nframes, d_rec + rec_index[k]) on the corrected
 *                bytes: stream k's block of d_rec, together with s, is what vit_data_groups_dev takes.
 * d_score, if not NULL: words 103k ... 103k+102 hold stream k's scores, 0 for streams of the other two modes; if NULL the
 * scores live in the calling thread's scratch.  d_srec[k] is written for every stream.  Bytes of d_bytes outside the
 * streams, FEC records beyond nfec and anything outside the named ranges are neither read nor written; the result does
 * not depend on scheduling.  The table is validated as by vit_packet_table_layout; then d_bytes, d_srec and d_rec must
 * not be NULL, d_srec, d_fec, d_rec and d_score must be 4-byte aligned, and d_fec may be NULL only when nfecrec is 0.
 * Everything is enqueued on `stream`: no host synchronisation and no device-to-host copy.
 * Launches, whatever nstreams: a clear of the scores; the sync, a workgroup per FEC_SEARCH stream and 1024 slots; the
 * pick, a wavefront per stream, which writes d_srec; the FEC, a workgroup per 20 frames of one stream, sized from the
 * bound nslots / 103 (the given phase's count for FEC_PHASE) - a workgroup whose first frame is not below nfec leaves at
 * once; the packets, a wavefront's round on 64 / (framebytes/24) logical frames of one stream.  A stage that no entry
 * uses is skipped (clear and sync without a FEC_SEARCH entry and without d_score; the FEC without a frame to decode). */
int vit_packet_table_dev(uint8_t *d_bytes, const vit_pkt_stream *h_tab, uint32_t nstreams,
                         vit_pkt_stream_rec *d_srec, vit_fec_rec *d_fec, vit_packet_rec *d_rec,
                         uint32_t *d_score /* uint32[103*nstreams], may be NULL */, void *stream);
/* Data groups for a whole ensemble: vit_data_groups_dev over up to 64 streams in one call, in a number of launches that
 * does not depend on the table's length - the stage behind vit_packet_table_dev, whose d_rec it takes as it stands
 * (rec_index = vit_pkt_layout.rec_index[k], offset = the packet table's offset).
 * Layout (vit_data_groups_table_layout): streams in table order; dg_index is the running sum of max_groups, data_offset
 * the running sum of data_capacity rounded up to a multiple of 16 (a records-only stream takes no room); ndg and
 * data_bytes are the sums' ends, bytes_end = max(offset + 24*nslots) and rec_end = max(rec_index + nslots).
 * Definition: stream k's records d_dg + dg_index[k], its summary d_sum[k] and its bytes d_data + data_offset[k] hold, byte
 * for byte, what
 *   vit_data_groups_dev(d_bytes + offset, d_rec + rec_index, nslots, d_dg + dg_index[k], max_groups, &d_sum[k],
 *                       records_only ? NULL : d_data + data_offset[k], data_capacity, stream)
 * writes there, and nothing else is written.  Every rule of that call holds per stream: first_slot, last_slot and
 * open_from count from the stream's own slot 0, a packet is usable only if it ends inside the stream's own nslots, groups
 * are numbered and placed per stream (offsets from the stream's block of d_data, multiples of 16), only the stream's
 * first nwritten records and the written groups' bytes are written, a stream with max_groups 0 still gets its summary, no
 * byte outside the streams' named ranges is read, and the result does not depend on scheduling.  The input is only read:
 * streams and record blocks may overlap or repeat; the layout keeps the outputs apart.  A NULL d_data makes every stream
 * records-only (it is allowed only where no stream asks for room).
 * Errors: VIT_ERR_NO_DEVICE first.  VIT_ERR_ARG, with vit_last_error() naming the entry, for nstreams outside 1 ... 64, an
 * nslots outside 1 ... 1<<24, records_only > 1, records_only 1 with a non-zero data_capacity, an offset + 24*nslots or
 * rec_index + nslots that does not fit 64 bits, more than 1<<26 slots in the table (the call keeps 16 bytes of scratch per
 * slot: 1 GiB there), or a dg_index or data_offset that would pass 2^32.  For the call also a NULL d_bytes, d_rec or
 * d_sum, a NULL d_dg with ndg > 0, a NULL d_data when some entry has records_only 0 and data_capacity > 0, or a d_rec,
 * d_dg or d_sum that is not 4-byte aligned.
 * Launches, whatever nstreams, all on `stream`, with no host synchronisation and no device-to-host copy: one clear of the
 * streams' scratch headers, then the kernels of vit_data_groups_dev with each workgroup's stream found from the table in
 * the kernel arguments - presence (a workgroup per 4096 slots of a stream); link totals (per address and chunk of 16384
 * slots but a stream's last; only if some stream has more than one chunk); link emit (per address and chunk); sums (a
 * workgroup per 4096 slots); bases (a workgroup per stream); place (as sums); gather (a wavefront per group that may be
 * written, max(1, min(max_groups, nslots)) per stream, at most 4096 of them; they number the groups that are written
 * through the table from the streams' counts and stride over them; wavefront k also writes stream k's summary).  Scratch
 * (the calling thread's): 256 bytes per stream and what vit_data_groups_dev takes for each. */
#define VIT_DG_MAX_STREAMS 64               /* = VIT_PKT_MAX_STREAMS */
typedef struct vit_dg_stream {              /* 32 bytes, host table entry */
    uint64_t offset;                        /* bytes from d_bytes to the stream's first byte; any alignment */
    uint64_t rec_index;                     /* the stream's first vit_packet_rec in d_rec */
    uint32_t nslots;                        /* 1 ... 1<<24 */
    uint32_t max_groups;                    /* as in vit_data_groups_dev; may be 0 */
    uint32_t data_capacity;                 /* as in vit_data_groups_dev */
    uint32_t records_only;                  /* 0, or 1 = this stream as with d_data NULL; then data_capacity must be 0 */
} vit_dg_stream;
typedef struct vit_dg_layout {
    uint64_t dg_index[VIT_DG_MAX_STREAMS];     /* first vit_dgroup_rec of stream k: running sum of max_groups */
    uint64_t data_offset[VIT_DG_MAX_STREAMS];  /* stream k's block of d_data: running sum of data_capacity rounded up to 16 */
    uint64_t ndg, data_bytes;                  /* sizes of d_dg (records) and d_data (bytes) */
    uint64_t bytes_end, rec_end;               /* what d_bytes (bytes) and d_rec (records) must hold */
} vit_dg_layout;
/* Host only, needs no GPU. */
int vit_data_groups_table_layout(const vit_dg_stream *h_tab, uint32_t nstreams, vit_dg_layout *h_out);
int vit_data_groups_table_dev(const uint8_t *d_bytes, const vit_packet_rec *d_rec, const vit_dg_stream *h_tab,
                              uint32_t nstreams, vit_dgroup_rec *d_dg, vit_dgroup_summary *d_sum /* [nstreams] */,
                              uint8_t *d_data /* may be NULL */, void *stream);

/* Multiplex configuration: from the FIBs that vit_decode_fic_dev leaves on the device to the sub-channel table that
 * vit_ensemble_dev takes - FIG 0/0 (ensemble identifier, CIF counter), FIG 0/1 (sub-channel organisation) and FIG 0/2
 * (which sub-channel carries which service component) of EN 300 401 clause 6, and the equal error protection profiles
 * of clause 11.3.2.  The definitions below are the library's, written without the standard's text at hand; they are
 * what these calls promise and what the tests check.  Each constant stands once in csrc/vit_fig_fmt.h.
 * Input: nfibs FIBs of 32 bytes back to back, the layout of d_fibs of vit_decode_fic_dev, at any alignment; only bytes
 * 0..29 of a FIB are parsed.  d_fib_ok[i] are the flags of vit_decode_fic_dev: a FIB whose flag is 0 is not looked at;
 * NULL means every FIB is used.  Group g holds the FIBs g*G ... min((g+1)*G, nfibs)-1, G = 1 ... 4096; there are
 * ngroups = ceil(nfibs/G) groups (G = 12: one mode-I transmission frame a group).
 *
 * The walk of one used FIB b[0..29]: position p = 0; while p < 30:
 *   h = b[p]; h == 0xFF ends the FIB.  type = h>>5, len = h&31.  If p+1+len > 30 the FIB is `malformed` and ends here.
 *   If type == 0 and len >= 1, the FIG body b[p+1 .. p+len] is examined as below.  In every case p += 1+len (len == 0
 *   advances one byte).
 * FIG type 0: t = b[p+1] holds C/N t>>7, OE (t>>6)&1, P/D (t>>5)&1 and the extension t&31.  Only extensions 0, 1 and 2
 * are read.  One of them with C/N or OE set (the next configuration, another ensemble) counts into n_next and is
 * otherwise passed over; status bits 2..4 are set by the others, whatever they turn out to hold.  Entries follow from
 * q = p+2 and end before e = p+1+len.
 *   extension 0   needs e-q >= 4, else `malformed`: EId b[q]<<8|b[q+1], change flags b[q+2]>>6, Al (b[q+2]>>5)&1, cif
 *                 (b[q+2]&31)<<8|b[q+3]; a fifth byte is ignored.
 *   extension 1   while q < e: fewer than 3 bytes left is `malformed` and ends the FIG.  SubChId b[q]>>2, start
 *                 (b[q]&3)<<8|b[q+1].  b[q+2]>>7 == 0, short form: table switch (b[q+2]>>6)&1, table index b[q+2]&63, 3
 *                 bytes.  b[q+2]>>7 == 1, long form: a missing 4th byte is `malformed` and ends the FIG; option
 *                 (b[q+2]>>4)&7, level (b[q+2]>>2)&3, size (b[q+2]&3)<<8|b[q+3], 4 bytes.
 *   extension 2   while q < e: a service identifier of 2 bytes (P/D 0) or 4 bytes (P/D 1), big-endian; one byte whose
 *                 low 4 bits are the component count nc; nc components of 2 bytes c0 c1 with TMId c0>>6.  TMId 0 and 1:
 *                 type c0&63, SubChId c1>>2, P/S (c1>>1)&1, CA c1&1 - one component entry.  TMId 2 and 3 give none.  If
 *                 the identifier with its count byte, or any of the nc components, does not fit before e, the FIG is
 *                 `malformed` and ends there; the components read before still count.
 * Packed words:
 *   org    bit 31 present, bit 30 long form, bits 9..0 start; long: bits 19..10 size, 21..20 level, 24..22 option;
 *          short: bits 15..10 table index, bit 16 table switch; other bits 0
 *   comp   bit 31 present, bits 1..0 TMId, bits 7..2 type, bit 8 P/S, bit 9 CA; other bits 0
 * Per group the entries are ordered by (FIB index, byte offset in the FIB), and the last entry for a SubChId wins - for
 * org and for (comp, sid) separately.  The result does not depend on scheduling: two runs give the same bytes.
 * A FIB holds at most 12 entries (a component costs 2 bytes behind 5 bytes of headers; a sub-channel 3, a FIG 0/0 six)
 * and at most 15 FIGs, so with G <= 4096 every count below stays inside 16 bits (49152, 61440). */
typedef struct vit_mci_subch {      /* 20 bytes; d_sub[g*64 + SubChId]; written completely, all 0 if never signalled */
    uint32_t org, comp, sid;
    uint16_t n_org, n_org_other;    /* FIG 0/1 entries of the group for this SubChId equal to / different from org */
    uint16_t n_comp, n_comp_other;  /* FIG 0/2 entries equal to / different from (comp, sid) */
} vit_mci_subch;
typedef struct vit_mci_group {      /* 16 bytes; written completely */
    uint16_t eid, cif;              /* of the last FIG 0/0 of the group */
    uint8_t  flags, reserved;       /* bit 0: a FIG 0/0 was seen, bits 2..1 change flags, bit 3 Al */
    uint16_t nfib_used, nfib_malformed;
    uint16_t n_ens_other;           /* FIG 0/0 entries whose (eid, change, Al) differ from the last one's */
    uint16_t n_next, reserved2;     /* FIGs 0/0..0/2 passed over for C/N or OE */
} vit_mci_group;
#define VIT_MCI_USED      0x01      /* d_status[i]: the FIB was walked (a FIB that is not used gets 0) */
#define VIT_MCI_MALFORMED 0x02
#define VIT_MCI_FIG00     0x04      /* a FIG 0/0, 0/1, 0/2 of the current configuration was read */
#define VIT_MCI_FIG01     0x08
#define VIT_MCI_FIG02     0x10
/* d_sub receives 64*ngroups records, d_grp ngroups, d_status (may be NULL) nfibs bytes.  Errors as the other *_dev
 * calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG with vit_last_error() for a NULL d_fibs, d_sub or d_grp, G outside
 * 1 ... 4096, a negative nfibs, or a d_sub / d_grp that is not 4-byte aligned.  nfibs == 0 returns VIT_OK and writes
 * nothing.  Everything is enqueued on `stream` without synchronising; d_fibs is only read, and no byte outside its
 * 32*nfibs bytes.  One launch: a wavefront per group for G <= 64, a workgroup per group over tiles of 256 FIBs above. */
int vit_mci_fibs_dev(const uint8_t *d_fibs, const uint8_t *d_fib_ok /* may be NULL */, int64_t nfibs, uint32_t G,
                     vit_mci_subch *d_sub, vit_mci_group *d_grp, uint8_t *d_status /* may be NULL */, void *stream);
/* Host only, needs no GPU: the same definition on host memory (no alignment rule; otherwise the same VIT_ERR_ARG). */
int vit_mci_fibs_host(const uint8_t *h_fibs, const uint8_t *h_fib_ok, int64_t nfibs, uint32_t G,
                      vit_mci_subch *h_sub, vit_mci_group *h_grp, uint8_t *h_status);
/* Host only: the profile of an EEP (long form) sub-channel of size_cu capacity units.  The library still compiles in no
 * puncturing vectors: keep_pi[i] is the caller's vector PI_(i+1) as a keep mask (see "Punctured input"), which must have
 * 8+i+1 one bits, and keep_tail the tail's, 12 one bits in its low 24 and none above; otherwise VIT_ERR_ARG.
 * Built-in rule, L counted in blocks of 32 trellis steps (128 mother-code bits):
 *   option 0 (A)  n = size_cu/12, /8, /6, /4 for level 0 ... 3; framebits = 192n; (L1, L2, PI1, PI2) =
 *                 level 0 (6n-3, 3, 24, 23); level 1 (5, 1, 13, 12) for n = 1, else (2n-3, 4n+3, 14, 13);
 *                 level 2 (6n-3, 3, 8, 7); level 3 (4n-3, 2n+3, 3, 2)
 *   option 1 (B)  n = size_cu/27, /21, /18, /15; framebits = 768n; L1 = 24n-3, L2 = 3; (PI1, PI2) = (10, 9), (6, 5),
 *                 (4, 3), (2, 1)
 * out receives the three segments {32*L1, PI1}, {32*L2, PI2}, {6, keep_tail}, *framebits the frame length.  VIT_ERR_ARG
 * also for a NULL pointer, option > 1, level > 3, a size_cu that is not a positive multiple of the unit, or framebits >
 * 9216.  Every result satisfies vit_punctured_length(out, *framebits) == 64*size_cu. */
int vit_eep_profile(uint32_t option, uint32_t level, uint32_t size_cu, const uint32_t keep_pi[24], uint32_t keep_tail,
                    vit_punct_profile *out, uint32_t *framebits);
/* Host only: the 64 records of one group -> rows for vit_ensemble_dev, SubChIds in ascending order.  A SubChId whose org
 * is present in long form, whose EEP profile builds (vit_eep_profile) and whose comp is present gives one row: col =
 * 64*start, framebits, nsym = 64*size, RSDims = framebits/192 if TMId 0 and type 63 (DAB+) else 0, profile = its index in
 * h_profiles (identical profiles are stored once), phase = nframes = reserved = 0 - superframe phase and batch length
 * stay the caller's, who fills them before vit_ensemble_layout.  Every other SubChId whose org is present - short form,
 * option > 1, a size the rule rejects, no component - sets bit SubChId of *skipped.  h_out has room for 64 rows, *nsub
 * receives their number; *nprofiles is the capacity of h_profiles going in and the number stored coming out.
 * VIT_ERR_ARG for a NULL pointer, vectors that vit_eep_profile rejects, or a capacity that is too small. */
int vit_mci_ens_table(const vit_mci_subch h_sub[64], const uint32_t keep_pi[24], uint32_t keep_tail,
                      vit_ens_subch *h_out, uint32_t *nsub, vit_punct_profile *h_profiles, uint32_t *nprofiles,
                      uint64_t *skipped);

/* Service directory: which services an ensemble carries, what they are called, and where their packet-mode components
 * lie - from the same FIBs, groups, d_fib_ok, G = 1 ... 4096 and ngroups as vit_mci_fibs_dev, whose FIG header rule
 * (p+1+len > 30 is `malformed` and ends the FIB; len == 0 advances one byte) and end marker hold unchanged.  It builds the
 * table that starts the packet chain (vit_packet_table_dev, vit_data_groups_table_dev) and ties a packet address to its
 * service.  As above, the layouts are the library's definitions, written without the standard's text at hand; each
 * constant stands once in csrc/vit_fig_fmt.h.
 *
 * The walk of one used FIB reads FIG type 0 extensions 2 and 3 and FIG type 1 extensions 0, 1 and 5, each only with
 * len >= 1; everything else is passed over by its length.  t = b[p+1]; the body ends before e = p+1+len, q = p+2.
 * A FIG 0/2 or 0/3 with C/N (t>>7) or OE ((t>>6)&1) set, and a FIG 1/0, 1/1 or 1/5 with bit 3 of t set, counts into n_next
 * and is otherwise passed over; the others set their status bit, whatever they turn out to hold.
 *   FIG 0/2   exactly the walk of vit_mci_fibs_dev: while q < e an identifier of 2 (P/D 0) or 4 (P/D 1) bytes, big-endian,
 *             a count byte, nc = count & 15 components c0 c1 of 2 bytes; an identifier with its count byte, or a
 *             component, that does not fit before e makes the FIG `malformed` and ends it; what was read before counts.
 *             Each service header gives one service entry: key SId, value (P/D, count byte).  Each component with TMId
 *             c0>>6 == 3 gives one component entry: key SCId = (c0&63)<<6 | c1>>2, value (SId, P/S (c1>>1)&1, CA c1&1).
 *             TMId 0, 1 and 2 give none here.
 *   FIG 0/3   while q < e: fewer than 5 bytes left is `malformed` and ends the FIG.  b = b[q ..]: SCId b0<<4 | b1>>4,
 *             CAOrg flag b1&1 (bits 3..1 of b1 are ignored), DG flag b2>>7, DSCTy b2&63, SubChId b3>>2, packet address
 *             (b3&3)<<8 | b4.  With the CAOrg flag set the entry has two more bytes, which are skipped; if they do not
 *             fit before e the FIG is `malformed` and ends there, and this entry gives nothing.  Each entry gives one
 *             location entry: key SCId, value loc (below).
 *   FIG 1     charset t>>4, extension t&7.  The identifier, big-endian, is 2 bytes for extensions 0 and 1 and 4 bytes for
 *             extension 5; 16 label bytes follow, then the 16-bit character flag field, big-endian.  len < 1 + idlen + 18
 *             is `malformed` (the FIG gives nothing; the walk goes on behind it); further bytes are ignored.  Extension 0
 *             gives the ensemble label entry: value (EId, label, chars, charset).  Extensions 1 and 5 give a label
 *             entry: key SId, value (label, chars, charset).
 * A 16-bit SId and a 32-bit SId share one 32-bit key space, compared as the numbers they are; P/D is part of the service
 * entry's value, not of the key.
 * Per group the entries are ordered by (FIB index, byte offset in the FIB).  For every key and kind the last entry wins;
 * the group's other entries of that key and kind are counted as equal to the winner or different from it.
 * Which keys get a record: the distinct SIds of the group's service and label entries, and separately the distinct
 * SCIds of its component and location entries, each set in ascending order; the first VIT_DIR_MAX of a set get records,
 * in that order.  If there are more the group's overflow flag for that table is set and the others leave no trace.
 * Records beyond the number written are all 0.  The result does not depend on scheduling: two runs give the same bytes.
 * A FIB holds at most 13 entries (one service header and 12 TMId-3 components), 9 service entries, 5 location entries,
 * 1 label and 15 FIGs, so with G <= 4096 every count below stays inside 16 bits. */
#define VIT_DIR_MAX 64
typedef struct vit_mci_service {   /* 32 bytes; d_svc[g*64 + i], ascending sid; written completely */
    uint32_t sid;
    uint8_t  label[16];
    uint16_t chars;                /* character flag field of the winning label */
    uint8_t  flags;                /* bit 0 a label was seen, bit 1 a FIG 0/2 service entry was seen,
                                      bit 2 P/D of the last one, bits 7..4 charset of the winning label */
    uint8_t  count;                /* count byte of the last FIG 0/2 service entry, as it stands */
    uint16_t n_label, n_label_other;     /* label entries equal to / different from the winner (label, chars, charset) */
    uint16_t n_listed, n_listed_other;   /* service entries equal to / different from (P/D, count byte) */
} vit_mci_service;
typedef struct vit_mci_pktcomp {   /* 20 bytes; d_pkt[g*64 + i], ascending scid; written completely */
    uint16_t scid;
    uint16_t flags;                /* bit 0 a FIG 0/3 entry was seen, bit 1 a TMId-3 component was seen,
                                      bit 2 P/S, bit 3 CA of the last one */
    uint32_t loc;                  /* last FIG 0/3 entry: bits 5..0 SubChId, 15..6 packet address, 21..16 DSCTy,
                                      bit 22 DG flag, bit 23 CAOrg flag; 0 if none */
    uint32_t sid;                  /* of the last TMId-3 component naming this SCId; 0 if none */
    uint16_t n_loc, n_loc_other, n_comp, n_comp_other;
} vit_mci_pktcomp;
typedef struct vit_mci_dir {       /* 40 bytes; d_dir[g]; written completely */
    uint16_t eid, chars;           /* of the last FIG 1/0 */
    uint8_t  label[16];
    uint8_t  flags;                /* bit 0 a FIG 1/0 was seen, bit 1 more than 64 SIds, bit 2 more than 64 SCIds */
    uint8_t  charset;
    uint16_t n_label, n_label_other;     /* FIG 1/0 entries equal to / different from (eid, label, chars, charset) */
    uint16_t nsvc, npkt;           /* records written in d_svc / d_pkt for this group */
    uint16_t nfib_used, nfib_malformed, n_next, reserved[2];   /* (two reserved fields: records of whole dwords) */
} vit_mci_dir;
#define VIT_MCI_DIR_USED      0x01  /* d_status[i] of vit_mci_dir_dev: the FIB was walked (a FIB that is not used gets 0) */
#define VIT_MCI_DIR_MALFORMED 0x02
#define VIT_MCI_DIR_FIG02     0x04  /* a FIG 0/2, a FIG 0/3, a FIG 1/0, 1/1 or 1/5 of the current configuration was read */
#define VIT_MCI_DIR_FIG03     0x08
#define VIT_MCI_DIR_FIG1      0x10
/* d_svc and d_pkt receive 64*ngroups records each, d_dir ngroups, d_status (may be NULL) nfibs bytes.  Argument rules and
 * errors are those of vit_mci_fibs_dev: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG with vit_last_error() for a NULL d_fibs,
 * d_svc, d_pkt or d_dir, G outside 1 ... 4096, a negative nfibs, or a d_svc / d_pkt / d_dir that is not 4-byte aligned.
 * nfibs == 0 returns VIT_OK and writes nothing.  Everything is enqueued on `stream` without synchronising; d_fibs may
 * have any alignment and is only read, and no byte outside its 32*nfibs bytes.  One launch, shaped as vit_mci_fibs_dev's;
 * a group of more than 256 FIBs is walked twice (csrc/vit_mci_dir.hip). */
int vit_mci_dir_dev(const uint8_t *d_fibs, const uint8_t *d_fib_ok /* may be NULL */, int64_t nfibs, uint32_t G,
                    vit_mci_service *d_svc, vit_mci_pktcomp *d_pkt, vit_mci_dir *d_dir,
                    uint8_t *d_status /* may be NULL */, void *stream);
/* Host only, needs no GPU: the same definition on host memory (no alignment rule; otherwise the same VIT_ERR_ARG). */
int vit_mci_dir_host(const uint8_t *h_fibs, const uint8_t *h_fib_ok, int64_t nfibs, uint32_t G,
                     vit_mci_service *h_svc, vit_mci_pktcomp *h_pkt, vit_mci_dir *h_dir, uint8_t *h_status);
/* Host only: vit_mci_ens_table with the packet-mode sub-channels.  Every row vit_mci_ens_table gives is given unchanged.
 * In addition a SubChId whose org is present in long form, whose EEP profile builds, which has NO comp and which at
 * least one of the npkt records with bit 0 of flags set names in loc (bits 5..0) gives one row with RSDims = 0; it is then
 * not in *skipped.  Rows stay in ascending SubChId order; bit (row index) of *packet_rows marks the added rows.  A
 * SubChId that has a comp stays as vit_mci_ens_table makes it and is not marked.  With npkt == 0 (h_pkt may then be
 * NULL) every output equals vit_mci_ens_table's and *packet_rows is 0.  VIT_ERR_ARG as vit_mci_ens_table, and for a NULL
 * packet_rows, a NULL h_pkt with npkt > 0, or npkt > VIT_DIR_MAX. */
int vit_mci_dir_ens_table(const vit_mci_subch h_sub[64], const vit_mci_pktcomp *h_pkt, uint32_t npkt,
                          const uint32_t keep_pi[24], uint32_t keep_tail, vit_ens_subch *h_out, uint32_t *nsub,
                          vit_punct_profile *h_profiles, uint32_t *nprofiles, uint64_t *skipped, uint64_t *packet_rows);
/* Host only: the stream table of vit_packet_table_dev from the rows above, once the caller has filled nframes and
 * vit_ensemble_layout has placed them: one vit_pkt_stream per marked row k, in row order, with offset =
 * h_layout->work_offset[k], framebytes = framebits/8, nframes the row's, the given fec, phase 0, min_score (used with
 * VIT_PKT_FEC_SEARCH; it must be 0 with VIT_PKT_FEC_NONE) and reserved 0.  h_out has room for 64 entries, *nstreams receives
 * their number (0 if no row is marked), h_row_of_stream[s], if not NULL, the row of stream s.  The FEC scheme is not read
 * from the FIC: fec is the caller's, VIT_PKT_FEC_NONE or VIT_PKT_FEC_SEARCH; VIT_PKT_FEC_PHASE is VIT_ERR_ARG, because
 * one phase does not fit several streams.  VIT_ERR_ARG also for a NULL pointer, nsub outside 1 ... 64, a bit of packet_rows
 * at or above nsub, a marked row whose RSDims is not 0, whose nframes is 0 or whose framebits/8 is no multiple of 24 in
 * 24 ... 1152, and a non-zero min_score with VIT_PKT_FEC_NONE.  A table of one stream or more passes
 * vit_packet_table_layout. */
int vit_mci_pkt_table(const vit_ens_subch *h_rows, uint32_t nsub, const vit_ens_layout *h_layout, uint64_t packet_rows,
                      uint32_t fec, uint32_t min_score, vit_pkt_stream h_out[64], uint32_t *nstreams,
                      uint32_t *h_row_of_stream /* may be NULL */);

/* From the FFT: differential demodulation, frequency de-interleaving, QPSK demapping and quantisation of whole
 * transmission frames (EN 300 401 clauses 14.5 - 14.7 seen from the receiver) - the step between an FFT on the device and
 * vit_decode_fic_dev / the ring of the *_ti_dev calls.
 * Input: the FFT outputs of whole frames, interleaved (re, im) float32, bin 0 = DC, in the order an FFT leaves them
 * (carrier k < 0 at bin nfft + k).  Symbol l of frame t starts at complex element t*frame_stride + l*sym_stride (strides
 * in complex elements, sym_stride >= nfft; the null symbol is the caller's to skip, which is what frame_stride is for).
 * Symbol 0 of a frame is the phase reference symbol, symbols 1 ... nsyms-1 are data.  d_fft must be 16-byte aligned and
 * both strides even (rocFFT output is).
 * The shape of a frame is a HOST struct, read during the call; no table of transmission modes is compiled in. */
typedef struct vit_ofdm_shape {
    uint32_t nfft;      /* FFT length; power of two, 64 ... 8192 */
    uint32_t ncarriers; /* K: QPSK symbols per OFDM symbol, 1 ... nfft; an OFDM symbol carries 2K bits */
    uint32_t nsyms;     /* OFDM symbols per frame in d_fft, phase reference included (mode I: 76); > fic_syms */
    uint32_t fic_syms;  /* the first fic_syms data symbols go to d_fic (mode I: 3) */
    uint32_t cifs;      /* CIFs per frame (mode I: 4), >= 1; (nsyms - 1 - fic_syms) must be a multiple of it */
} vit_ofdm_shape;
/* mode I {2048,1536,76,3,4}, II {512,384,76,3,1}, III {256,192,153,8,1}, IV {1024,768,76,3,2} */
/* Frequency de-interleaving is a caller-supplied DEVICE table d_bins[K]: QPSK symbol n of an OFDM symbol is carried by
 * FFT bin d_bins[n].  The table is only read on the device, so it is checked there: its entries must be < nfft and
 * distinct (a carrier bears one QPSK symbol).  For a table that breaks this the bytes of the carriers involved are
 * unspecified, but nothing outside the rows of d_fft is read and nothing outside the call's own output bytes is written.
 * The standard's table, a built-in definition like the PRBS and F (EN 300 401 clause 14.6):
 * Host only, needs no GPU.  P(0) = 0, P(i) = (13*P(i-1) + nfft/4 - 1) mod nfft for i = 1 ... nfft-1; the values with
 * nfft/8 <= P(i) <= 7*nfft/8 and P(i) != nfft/2, in the order they occur, are d_0 ... d_{K-1}, K = 3*nfft/4; QPSK
 * symbol n travels on carrier k = d_n - nfft/2, i.e. FFT bin k mod nfft.  Writes K bins to h_bins and returns K,
 * or -1 for nfft not in {256, 512, 1024, 2048} or a NULL pointer. */
int64_t vit_freq_interleave_bins(uint32_t nfft, uint16_t *h_bins);
/* Per data symbol l = 1 ... nsyms-1 of frame t and per n = 0 ... K-1, with a = z[t, l, d_bins[n]] and
 * b = z[t, l-1, d_bins[n]], every operation an IEEE binary32 operation rounded to nearest-even, in exactly this order,
 * never contracted into an FMA:
 *   re  = fl(fl(a.re*b.re) + fl(a.im*b.im))          y = a * conj(b): pi/4-DQPSK leaves y on a diagonal,
 *   im  = fl(fl(a.im*b.re) - fl(a.re*b.im))          re(y) > 0 <=> bit n = 0, im(y) > 0 <=> bit n+K = 0
 *   nrm = fl(|re| + |im|)
 *   if not (2^-64 <= nrm <= FLT_MAX):   out[n] = out[n+K] = 128        (no signal, NaN, Inf: erasures)
 *   else  s = fl(gain / nrm)
 *         out[n]   = clamp(128 - rint(fl(re*s)), 0, 255)
 *         out[n+K] = clamp(128 - rint(fl(im*s)), 0, 255)               rint: ties to even
 * gain: a host float, finite, 0 < gain <= 65536; an ideal constellation point gives 128 -/+ gain/2, so 254 uses the whole
 * byte range there.  Normalising per carrier by |re| + |im| needs no reduction, so the result is defined bit for bit; the
 * lower bound on nrm makes a muted carrier an erasure and keeps the result independent of how denormals are handled.
 * Where the 2K bytes `out` of data symbol s = l-1 of frame t go:
 *   s < fic_syms:  d_fic + (t*fic_syms + s) * 2K.  In modes I, II and IV a frame's fic_syms*2K bytes are whole blocks of
 *                  2304 transmitted symbols: the input of vit_decode_fic_dev(..., 768, ..., &fic_profile, ...).
 *   otherwise:     with m = s - fic_syms and per = (nsyms-1-fic_syms)/cifs, CIF c = m / per of the frame: ring row
 *                  (first_row + t*cifs + c) mod nrows, columns col + (m mod per)*2K ...  With the rows of mode I
 *                  (per*2K = 55296) that is the ring of the *_ti_dev calls, and first_row advances by nframes*cifs from
 *                  call to call.
 * This call is the ring's WRITER: it writes through ring->d_base (the struct keeps its `const` for the readers).
 * d_fic may be NULL: the FIC symbols are not demapped.  ring may be NULL: the MSC symbols are not demapped and their rows
 * of d_fft not read.
 * Argument rules as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL
 * d_fft / d_bins / shape, both destinations NULL, a misaligned d_fft or an odd stride, sym_stride < nfft, an invalid shape
 * or gain, nframes < 0, a ring with a NULL d_base, first_row >= nrows, nframes*cifs > nrows (the call's rows must be
 * distinct), col + per*2K > row_bytes; an empty batch returns VIT_OK and writes nothing; everything is enqueued on
 * `stream` without synchronising.
 * Guarantees: no byte is written outside the bytes named above (d_fic, the ring, col and row_bytes may have any
 * alignment); no bin that d_bins does not name influences any output (guard bins and DC may hold NaN); ring rows other
 * than the call's nframes*cifs rows - the 15-row overlap of a streaming ring among them - are never touched. */
int vit_ofdm_demap_dev(const float *d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t *d_bins,
                       const vit_ofdm_shape *shape, float gain, int64_t nframes, uint8_t *d_fic,
                       const vit_cif_ring *ring, uint64_t col, void *stream);

/* From the samples: fine-frequency correction, the FFT of every OFDM symbol and, fused behind it, exactly what
 * vit_ofdm_demap_dev does - the step between baseband samples on the device and vit_decode_fic_dev / the ring, with no
 * spectrum written to memory and no third-party FFT in the caller's hot path.  Like the demapper it is defined bit for bit.
 * Input: a HOST struct, read during the call (like vit_cif_ring).  A frame's "start" is the first useful sample of its
 * phase reference symbol (the caller places it inside the guard interval as its time synchronisation says); the useful
 * part of symbol l of frame t is samples start_t + l*sym_stride ... + nfft - 1.  Nothing else is read: not the samples
 * between useful parts, not the null symbol.  Any sample position is allowed; only d_iq must be 8-byte aligned.
 * The two tables come from vit_ofdm_sync_dev ("From the coarse start", below) or from the caller's own estimator.
 * Integer samples as receivers deliver them go through the *_iq_dev calls ("Integer sample formats", below).
 * Channel-state weighting is a second soft-decision rule of both demappers ("Channel-state weighting", below).
 * First acquisition (finding the null symbol) is vit_ofdm_acquire_dev ("From the stream", below).  A stream at another
 * sample rate, or one that holds several ensembles, goes through vit_iq_resample_dev first ("Before the stream", below). */
typedef struct vit_iq_input {
    const float    *d_iq;         /* interleaved (re, im) float32 samples, 8-byte aligned (*_iq_dev: samples of fmt->format) */
    uint64_t        nsamples;     /* complex samples in d_iq: nothing at or beyond it is read */
    uint64_t        sym_stride;   /* samples from one symbol's useful part to the next: nfft + guard (mode I 2552), >= nfft */
    uint64_t        frame_stride; /* frame t starts at sample t*frame_stride when d_start is NULL (mode I 196608) */
    const int64_t  *d_start;      /* optional DEVICE table: frame t starts at sample d_start[t] (timing re-estimated per frame) */
    const float    *d_tw;         /* DEVICE: nfft/2 twiddles, from vit_fft_twiddles */
    const float    *d_nco;        /* optional DEVICE: 2^nco_bits phasors, from vit_nco_table */
    uint32_t        nco_bits;     /* 1 ... 20 */
    const uint32_t *d_rot;        /* optional DEVICE: per frame {phase0, step}; NULL = no rotation, not even by 1 */
} vit_iq_input;
/* Definition.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly this order, never
 * contracted into an FMA; tw and nco are the caller's tables (the builders below give the intended ones).
 * 1. Rotation, only if d_rot is given.  Sample n of a frame is counted from the frame's start, guards included:
 *    n = l*sym_stride + i for sample i of symbol l, so the phase is continuous across the frame.  With
 *    w = nco[((phase0 + n*step) mod 2^32) >> (32 - nco_bits)]:
 *      x'.re = fl(fl(x.re*w.re) - fl(x.im*w.im))
 *      x'.im = fl(fl(x.re*w.im) + fl(x.im*w.re))
 *    The caller sets step = round(-df/fs * 2^32) mod 2^32 for a frequency offset df at sample rate fs.
 * 2. FFT, nfft = 2^m: radix-2 decimation in time.  x0[i] = x'[bitrev_m(i)].  For stage s = 1 ... m, with h = 2^(s-1),
 *    for every block base i (a multiple of 2^s) and j < h:
 *      w = tw[j * (nfft >> s)],  u = x[i+j],  v = x[i+j+h]
 *      t.re = fl(fl(w.re*v.re) - fl(w.im*v.im))
 *      t.im = fl(fl(w.re*v.im) + fl(w.im*v.re))
 *      x[i+j] = u + t,  x[i+j+h] = u - t            component by component
 *    The result is X[k] in FFT order: bin 0 = DC, carrier k < 0 at bin nfft + k.
 *    This pins the arithmetic graph, not an implementation: any grouping of stages and any memory layout compute the same
 *    bits as long as the same butterflies meet the same twiddles.
 * 3. Demapping (vit_ofdm_demod_dev): the definition of vit_ofdm_demap_dev unchanged, with z = X.
 * Domain: the result is defined for samples that are 0 or have a magnitude in [2^-40, 2^40].  There no
 * product with a table entry is denormal and nothing overflows before the demapper, whose own rules then take care of
 * Inf.  For a symbol that holds anything else (NaN, Inf, denormals, larger magnitudes) the outputs of that symbol and of
 * the next are unspecified; nothing is written outside the call's output bytes.  (So an implementation may skip the
 * multiplications by the exact table entries 1 and -j.)  The sign of a zero influences no output byte; spectra are
 * defined by value (-0 = +0).
 * Tables, host only, need no GPU (like vit_freq_interleave_bins).  Both compute in binary64 and round to binary32, except
 * that entries at multiples of an eighth of a turn are exact: 0, +-1, +-fl(sqrt(1/2)).  Each returns the number of pairs
 * written, or -1 for a NULL pointer or an argument out of range.
 *   vit_fft_twiddles: nfft/2 pairs (cos, -sin)(2 pi k / nfft), nfft a power of two 64 ... 8192
 *   vit_nco_table:    2^nco_bits pairs (cos, +sin)(2 pi k / 2^nco_bits), nco_bits 1 ... 20 */
int64_t vit_fft_twiddles(uint32_t nfft, float *h_tw);
int64_t vit_nco_table(uint32_t nco_bits, float *h_nco);
/* vit_ofdm_fft_dev: steps 1 and 2 for symbols 0 ... nsyms-1 of nframes frames; X of symbol l of frame t goes to complex
 * elements t*out_frame_stride + l*out_sym_stride ... + nfft - 1 of d_fft, the layout vit_ofdm_demap_dev reads (d_fft
 * 16-byte aligned, both output strides even, out_sym_stride >= nfft); nothing else of d_fft is written.  For callers
 * that need a spectrum (a channel estimate, an estimator of their own; vit_ofdm_sync_dev needs none).
 * vit_ofdm_demod_dev: steps 1 to 3; d_bins, shape, gain, d_fic, ring and col as in vit_ofdm_demap_dev, with the same
 * destinations, rules and guarantees (no write outside the named bytes, other ring rows untouched, no bin that d_bins
 * does not name influences any output).
 * Argument rules as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL `in`,
 * d_iq, d_tw or output, a d_iq, d_tw, d_nco, d_start or d_rot that is not 8-byte aligned, sym_stride < nfft, nfft not a power of two 64 ... 8192, nsyms = 0, d_rot
 * without d_nco or with nco_bits outside 1 ... 20, nframes < 0, and every rule of vit_ofdm_demap_dev for the outputs.
 * A frame's reads are taken to span all its symbols, start ... start + (nsyms-1)*sym_stride + nfft - 1, whichever of
 * them the call needs.  With d_start == NULL a last frame that would read beyond nsamples is VIT_ERR_ARG.  With d_start
 * given, a frame whose reads would fall outside [0, nsamples) is skipped on the device: every output byte of that
 * frame keeps its old value (the rule vit_decode_varlen_dev_checked has for its table).  An empty batch returns VIT_OK
 * and writes nothing; everything is enqueued on `stream` without synchronising. */
int vit_ofdm_fft_dev(const vit_iq_input *in, uint32_t nfft, uint32_t nsyms, int64_t nframes, float *d_fft,
                     uint64_t out_sym_stride, uint64_t out_frame_stride, void *stream);
int vit_ofdm_demod_dev(const vit_iq_input *in, const uint16_t *d_bins, const vit_ofdm_shape *shape, float gain,
                       int64_t nframes, uint8_t *d_fic, const vit_cif_ring *ring, uint64_t col, void *stream);

/* From the coarse start: fine time and frequency.  One call reads the samples and writes exactly the two per-frame DEVICE
 * tables vit_ofdm_demod_dev reads - d_start[t] and d_rot[t] = {phase0, step} - so nothing leaves the device between the
 * samples and the soft bytes.  It is the per-frame TRACKING step: it starts from a coarse start c that is right to within
 * +-W samples (the previous frame's start plus frame_stride, or the caller's null-symbol search) and a carrier offset of
 * less than M + 1/2 carrier spacings.  First acquisition (finding the null symbol in an unaligned stream) is
 * vit_ofdm_acquire_dev ("From the stream", below), which writes such a coarse table.  The transmitted phase reference symbol is a caller-supplied DEVICE table d_prs: nfft complex binary32 values
 * in FFT order, zero on unused bins (the library still holds no table of the standard except the bin table).
 * Like the rest of the front end the result is defined bit for bit. */
typedef struct vit_sync_params {
    uint32_t nfft;        /* power of two 64 ... 8192 */
    uint32_t nsyms;       /* symbols per frame incl. the phase reference (read span, skip rule); >= 2 */
    uint32_t cp_symbols;  /* guards used for the fractional estimate: those in front of symbols 1 ... cp_symbols; 1 ... nsyms-1 */
    uint32_t W;           /* timing uncertainty, samples; 2*W < guard and 2*W < nfft, guard = in->sym_stride - nfft < 2^31 */
    uint32_t M;           /* integer carrier offsets searched: -M ... M; 0 ... 64, 2*M < nfft */
    float    thr;         /* first-path threshold, (0, 1]; 1 = the strongest path */
    int32_t  backoff;     /* samples subtracted from the found start (places it inside the guard) */
    int64_t  first_start; /* coarse start of frame t = first_start + t*frame_stride when in->d_start is NULL */
} vit_sync_params;
/* Definition.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly this order, never
 * contracted into an FMA.  x: the samples; S = sym_stride, G = S - nfft, c = the frame's coarse start (in->d_start[t] or
 * first_start + t*frame_stride); P = d_prs; tw, nco: the tables of vit_iq_input.  Products of complex values:
 *   a * conj(b) = ( fl(fl(a.re*b.re) + fl(a.im*b.im)),  fl(fl(a.im*b.re) - fl(a.re*b.im)) )
 * Long sums.  NACC = max(64, nfft/8) accumulators start at +0; element e of a sum (e = 0, 1, ... in the order given) is
 * added to accumulator e mod NACC, in ascending e: acc = fl(acc + element), component by component.  Then the
 * accumulators meet in the tree of adjacent pairs: v[i] = fl(v[2i] + v[2i+1]) until one value is left.  The grouping
 * depends on nfft alone - never on nframes, the launch or the device.
 * A. Fractional offset.  Elements (l, k), l = 1 ... cp_symbols, k = 0 ... G-2W-1, l-major: e = (l-1)*(G-2W) + k, with
 *    n = c + l*S - G + W + k (inside the guard of symbol l wherever the true start lies in c +- W), a = x[n], b = x[n+nfft]:
 *      gamma += conj(a) * b = ( fl(fl(a.re*b.re) + fl(a.im*b.im)),  fl(fl(a.re*b.im) - fl(a.im*b.re)) )
 *      E     += fl( fl(fl(a.re*a.re) + fl(a.im*a.im)) + fl(fl(b.re*b.re) + fl(b.im*b.im)) )
 *    turn = atan2(gamma.im, gamma.re) / 2 pi in [-1/2, 1/2] by this graph: ax = |gamma.re|, ay = |gamma.im|,
 *    mx = max(ax, ay), mn = min(ax, ay); mx = 0 gives turn = 0; else q = fl(mn / mx), s = fl(q*q),
 *      p = C6;  p = fl(fl(p*s) + Ci) for i = 5 ... 0;  r = fl(p*q)                  (r = atan(q) / 2 pi, 0 ... 1/8)
 *      if ay > ax: r = fl(0.25 - r);   if gamma.re < 0: r = fl(0.5 - r);   if gamma.im < 0: r = -r;   turn = r
 *    with the coefficients below (error of the graph against atan2: under 2^-23 turn).
 *      step_frac = (-rint(fl(turn * 2^32/nfft))) mod 2^32                      rint: ties to even; the product is exact
 * B. Phase reference spectrum.  The window starts at w0 = c - W.  Sample i < nfft, x[w0 + i], is rotated as in step 1 of
 *    "From the samples" with phase0 = 0, step = step_frac, n = i; Y = the FFT of step 2 of it.
 * C. Integer offset.  D[k] = Y[k] * conj(Y[k-1]), R[k] = P[k] * conj(P[k-1]), indices mod nfft.  For m = -M ... M:
 *      C[m] = sum over k = 0 ... nfft-1 (a long sum, e = k) of D[(k+m) mod nfft] * conj(R[k])
 *      metric[m] = fl(fl(C.re*C.re) + fl(C.im*C.im))
 *    m^ = the first maximum in the order -M ... M (a later m replaces it only if its metric is greater).
 * D. Timing.  Z[k] = Y[(k+m^) mod nfft] * conj(P[k]);  h = conj(FFT(conj Z)), the same FFT graph, no scaling;
 *      p[n] = fl(fl(h.re*h.re) + fl(h.im*h.im));   psum = the long sum of p[n], e = n = 0 ... nfft-1
 *      pmax = max of p[0 ... 2W];   tau = the first n <= 2W with p[n] >= fl(thr * pmax)
 * E. Outputs.  d_start_out[t] = c - W + tau - backoff;   d_rot_out[t] = {0, (step_frac - m^ * (2^32/nfft)) mod 2^32};
 *    d_info[8t ...] = {int32 m^, int32 tau, gamma.re, gamma.im, E, metric[m^], pmax, psum}  (optional: quality figures -
 *    |gamma| / (E/2) is the guard correlation, pmax / psum the share of the first paths' power).
 * Domain: the samples' domain of "From the samples", and no operation above overflows - with |P[k]| <= 1 that holds for
 * sample magnitudes up to 2^12 at every nfft.  Underflow is gradual: denormal results are kept, as IEEE arithmetic has
 * them.  All-zero samples are inside the domain: every comparison ties, m^ = -M, tau = 0, turn = 0.  Outside it the
 * frame's outputs are unspecified; nothing but the call's output words is written.
 * One extension of that domain, for step A alone: a sample that no transform reads - one outside the window of step B,
 * c - W ... c - W + nfft - 1, so a guard pair of symbols 1 ... cp_symbols - may have any finite value for which nothing
 * overflows, magnitudes under 2^-40 and denormals included.  Step A multiplies samples with samples only and meets no
 * table; gamma, E, q, the polynomial and turn are then what IEEE arithmetic gives, a denormal or zero q and a denormal
 * turn among them.  Every sample inside the window of step B keeps the floor of "From the samples": 0 or 2^-40 and more.
 * The accumulators start at +0, so gamma.im is never -0: gamma.re < 0 with gamma.im = 0 gives turn = +1/2 and
 * step_frac * nfft = 2^31 mod 2^32; a gamma.im < 0 too small to change fl(0.5 - r) gives turn = -1/2.  thr may be any
 * positive binary32 value, denormal included; fl(thr * pmax) may be denormal, and where it rounds to 0, tau = 0.
 * Skip rule: a frame's reads are taken to span c - W ... c + (nsyms-1)*S + nfft - 1 + W.  With in->d_start given, a frame
 * whose span is not inside [0, nsamples) is skipped on the device: it gets start -1, rot {0, 0} and info zeros, so
 * vit_ofdm_demod_dev skips it too by its own rule.  Without in->d_start such a frame is VIT_ERR_ARG.
 * in: the struct vit_ofdm_demod_dev takes.  in->d_start, if given, is the coarse table (d_start_out may be the same
 * pointer); in->d_nco and in->nco_bits are required; in->d_rot must be NULL.  d_info may be NULL.
 * Argument rules as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL in, p,
 * d_iq, d_tw, d_nco, d_prs, d_start_out or d_rot_out; a d_iq, d_tw, d_nco, d_start, d_prs, d_start_out or d_rot_out that is
 * not 8-byte aligned or a d_info that is not 4-byte aligned; nco_bits outside 1 ... 20; in->d_rot set; every range in the
 * struct's comments (2*W >= guard among them); a span beyond 2^64 samples; nframes < 0.  An empty batch returns VIT_OK and
 * writes nothing; everything is enqueued on `stream` without synchronising. */
#define VIT_SYNC_ATAN_C0  0x1.45f2b4p-3f
#define VIT_SYNC_ATAN_C1 -0x1.b26414p-5f
#define VIT_SYNC_ATAN_C2  0x1.0240f6p-5f
#define VIT_SYNC_ATAN_C3 -0x1.591268p-6f
#define VIT_SYNC_ATAN_C4  0x1.9f40a4p-7f
#define VIT_SYNC_ATAN_C5 -0x1.5e8136p-8f
#define VIT_SYNC_ATAN_C6  0x1.1c32c4p-10f
int vit_ofdm_sync_dev(const vit_iq_input *in, const vit_sync_params *p, const float *d_prs, int64_t nframes,
                      int64_t *d_start_out, uint32_t *d_rot_out, uint32_t *d_info, void *stream);

/* Integer sample formats: the front end reads the receiver's own buffer.  An RTL-SDR delivers unsigned 8-bit pairs, a
 * HackRF signed 8-bit, Airspy, SDRplay and USRP signed 16-bit; the *_iq_dev calls read them where the existing calls read
 * float32, so no float copy of the stream exists on the device.  in->d_iq then points at samples of the named format (the
 * caller casts); nsamples, sym_stride, frame_stride, d_start and every position keep counting COMPLEX samples. */
#define VIT_IQ_F32  0   /* interleaved float32 (re, im): what the existing calls read */
#define VIT_IQ_CU8  1   /* bytes (I, Q), unsigned, offset 127.5 */
#define VIT_IQ_CS8  2   /* bytes (I, Q), two's complement */
#define VIT_IQ_CS16 3   /* int16 (I, Q), little endian */
typedef struct vit_iq_format {
    uint32_t format;      /* VIT_IQ_* */
    float    scale;       /* integer formats: finite, 2^-32 <= scale <= 2^16; VIT_IQ_F32: ignored, not even validated */
} vit_iq_format;
/* Definition: one line in front of step 1 of "From the samples" and of step A of "From the coarse start".  The binary32
 * value of a component is
 *   CU8:  fl( (float)(2*b - 255) * scale )  for byte b: the integer -255 ... 255 is exact in binary32, so there is one
 *         rounding; the usual (b - 127.5)/128 is scale = 2^-8.  No CU8 sample is ever 0.
 *   CS8:  fl( (float)b * scale )            for the two's complement byte b
 *   CS16: fl( (float)h * scale )            for the int16 h
 *   F32:  the value itself.
 * Everything downstream is the existing definition applied to these floats: the result of an *_iq_dev call equals, in
 * every output bit, the result of the existing call on the converted floats, and with VIT_IQ_F32 it is the existing call.
 * Domain: the scale's range keeps every nonzero component inside [2^-40, 2^40] for all three integer formats; the bound
 * of 2^12 of vit_ofdm_sync_dev stays the caller's to respect.  All-zero CS8 / CS16 symbols are inside the domain.
 * Arguments after fmt: exactly those of the call without _iq, with its rules, its read and skip rules counted in samples,
 * and its guarantees.  In addition VIT_ERR_ARG (with vit_last_error()) for a NULL fmt, an unknown format, or - for an
 * integer format - a scale outside its range (NaN included).  d_iq must be 4-byte aligned for the integer formats (8-byte
 * for VIT_IQ_F32); sample positions stay arbitrary: a CU8 frame may start at an address that is 2 mod 4.  No byte outside
 * the samples the float32 path would read influences an output, and nothing at or beyond nsamples is read.
 * vit_iq_convert_dev writes the 2*nsamples floats of the definition to d_out (8-byte aligned), for callers who need the
 * floats themselves (an estimator of their own, other consumers of vit_ofdm_fft_dev's input).  VIT_IQ_F32 is VIT_ERR_ARG:
 * there is nothing to convert.  nsamples = 0 returns VIT_OK and writes nothing; enqueued on `stream` without synchronising. */
int vit_ofdm_fft_iq_dev(const vit_iq_input *in, const vit_iq_format *fmt, uint32_t nfft, uint32_t nsyms, int64_t nframes,
                        float *d_fft, uint64_t out_sym_stride, uint64_t out_frame_stride, void *stream);
int vit_ofdm_demod_iq_dev(const vit_iq_input *in, const vit_iq_format *fmt, const uint16_t *d_bins,
                          const vit_ofdm_shape *shape, float gain, int64_t nframes, uint8_t *d_fic,
                          const vit_cif_ring *ring, uint64_t col, void *stream);
int vit_ofdm_sync_iq_dev(const vit_iq_input *in, const vit_iq_format *fmt, const vit_sync_params *p, const float *d_prs,
                         int64_t nframes, int64_t *d_start_out, uint32_t *d_rot_out, uint32_t *d_info, void *stream);
int vit_iq_convert_dev(const void *d_iq, const vit_iq_format *fmt, uint64_t nsamples, float *d_out, void *stream);

/* Before the stream: rate conversion and channel selection.  Every stage from vit_ofdm_acquire_dev on takes a stream at
 * the chain's sample rate (2.048 MS/s for DAB) that is centred on one ensemble.  Receivers deliver something else: an
 * Airspy 2.5, 3, 6 or 10 MS/s, a USRP 2.0 or 2.5 MS/s, and a 6 or 10 MS/s capture covers three to five DAB blocks at once.
 * One call shifts, low-pass filters and changes the rate by the rational factor L/M: it reads one stream - float32 or an
 * integer format of "Integer sample formats", which is why the section stands behind it - once and writes nchan float32
 * streams, each one ready for vit_ofdm_acquire_dev (d_out + 2*c*out_stride is channel c's d_iq).  It is a polyphase FIR
 * filter with caller-supplied taps (the library holds no table of the standard; a host builder below gives
 * windowed-sinc taps).  Like the rest of the front end the result is defined bit for bit. */
#define VIT_RESAMPLE_MAX_CHAN 16
typedef struct vit_resample_params {
    uint32_t L, M;        /* output rate = input rate * L / M; 1 <= L <= 1024, 1 <= M <= 4096 (need not be coprime) */
    uint32_t T;           /* taps per phase: a multiple of 4, 4 ... 128; L*T <= 16384 */
    uint32_t nchan;       /* 1 ... VIT_RESAMPLE_MAX_CHAN */
    uint64_t pos0;        /* position of output 0 in units of 1/L input sample (stream continuation, below) */
    const float *d_taps;  /* DEVICE: L*T floats, phase-major g[phi*T + k], from vit_resample_taps or the caller's own */
    const float *d_nco;   /* DEVICE: 2^nco_bits phasors from vit_nco_table; required iff rot != NULL */
    uint32_t nco_bits;    /* 1 ... 20 (read only when rot is given) */
    uint32_t reserved;    /* 0 */
    const uint32_t *rot;  /* HOST, read during the call: nchan pairs {phase0, step}; NULL = no rotation, nchan must be 1 */
} vit_resample_params;
/* Definition.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly this order, never
 * contracted into an FMA.  L, M, T, nchan, pos0, rot: the struct's; g = d_taps, nco = d_nco.
 * A. Sample.  x[n], n = 0 ... nsamples-1, is sample n of d_iq as binary32: the value itself for float32, components from
 *    the integer formats by the one-rounding rule of "Integer sample formats".
 * B. Rotation, channel c, only if rot is given.  With {phase0, step} = rot[2c], rot[2c+1] and n the index into d_iq, of
 *    which only the low 32 bits matter:
 *      w = nco[((phase0 + n*step) mod 2^32) >> (32 - nco_bits)]
 *      y.re = fl(fl(x.re*w.re) - fl(x.im*w.im))
 *      y.im = fl(fl(x.re*w.im) + fl(x.im*w.re))
 *    the graph of step 1 of "From the samples"; step = round(-f/fs * 2^32) mod 2^32 moves a channel centred at f, at input
 *    rate fs, to 0.  Without rot, y = x: no rotation, not even by 1.
 * C. Filter.  Output m, 0 <= m < nout, has P = pos0 + m*M in 64-bit arithmetic, n0 = P div L, phi = P mod L.  For each of
 *    the two components:
 *      term[k] = fl(g[phi*T + k] * y[n0 + k]),  k = 0 ... T-1
 *      four accumulators a0 ... a3 start at +0; in ascending k, term[k] is added to accumulator k mod 4: a = fl(a + term[k])
 *      result = fl( fl(a0 + a1) + fl(a2 + a3) )
 *    It is written to complex element c*out_stride + m of d_out (floats 2*(c*out_stride + m) and the next).  Results are
 *    defined by value (-0 = +0).
 * D. Reads and writes.  Output m reads samples n0 ... n0 + T - 1 and nothing else: no sample at or beyond nsamples is read,
 *    and none that no requested output needs - not in front of the first output's n0, not behind the last one's
 *    n0 + T - 1, not in a gap between two outputs' samples (M > L*T).  Only the nchan*nout named complex elements of d_out
 *    are written: not the gaps between channels when out_stride > nout.
 * The result depends on the samples, the tables and the struct alone: never on nout (output m has the same bits in every
 * call that reaches it), never on nchan (channel c has the same bits alone, with nchan = 1 and its own pair, or among
 * others), never on the launch or the device.
 * Stream continuation.  A caller who has consumed outputs 0 ... m1-1 and drops the first s = (pos0 + m1*M) div L samples of
 * the buffer (any s up to that; this is the most) calls again with
 *      pos0'   = (pos0 + m1*M) - s*L
 *      phase0' = (phase0 + s*step) mod 2^32     for every channel
 * on the buffer that starts at the old sample s: output m of the second call equals, bit for bit, output m1 + m of one long
 * call.  (n0 and n move by s together; phi, and the phase of every sample, stay.)
 * Timing.  Output m sits at input time (pos0 + m*M)/L + d, d the delay of the taps; the taps of vit_resample_taps have
 * d = T/2 - 1 input samples at every phase, a constant the caller adds to its start tables (in output samples: d*L/M).
 * Domain: every component of a sample is 0 or has a magnitude in [2^-40, 2^12] - the domain of vit_ofdm_acquire_dev and
 * vit_ofdm_sync_dev, which read the output; the taps are finite with |g| <= 4.  Then nothing overflows: a rotated
 * component is under 2^13, a term under 2^15, an accumulator under 32 * 2^15 and the result under 2^22.  Underflow is
 * gradual: denormal products and sums are kept as IEEE arithmetic has them, as in step A of vit_ofdm_sync_dev.  All-zero
 * samples are inside the domain and give zeros.  Outside the domain the outputs that read such samples are unspecified;
 * nothing but the named output words is written.
 * Host helpers, no GPU (like vit_fft_twiddles):
 *   vit_resample_out_count(nsamples, p): the largest nout for which the last output's n0 + T <= nsamples (and its P fits 64
 *     bits), clamped to 2^63 - 1; 0 if there is none (nsamples < T among the reasons); -1 for a NULL pointer or L, M, T
 *     outside their ranges.  It reads L, M, T and pos0 only.
 *   vit_resample_taps(L, T, cutoff, h_taps): a Blackman-windowed sinc, computed in binary64 and rounded to binary32.  For
 *     phase phi and tap k, with u = k - (T/2 - 1) - phi/L and sinc(x) = sin(pi x)/(pi x), sinc(0) = 1:
 *       h = 2*cutoff * sinc(2*cutoff*u) * (0.42 + 0.5 cos(2 pi u / T) + 0.08 cos(4 pi u / T))
 *     Each phase's T values are divided by their binary64 sum (ascending k), so the gain at DC is 1 at every phase, and
 *     then rounded.  cutoff is in cycles per INPUT sample, 0 < cutoff <= 0.5: when the rate goes down it must lie
 *     under half the OUTPUT rate, L/(2M).  Returns L*T, or -1 for a NULL pointer or an argument out of range (L, T as in
 *     the struct).
 * Arguments as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL d_iq, p,
 * d_taps or d_out; a d_iq that is not aligned as in "Integer sample formats" (8 bytes for float32, 4 for an integer
 * format); a d_taps, d_nco or d_out that is not 8-byte aligned; every range in the struct's comments; a nonzero reserved;
 * rot without d_nco, d_nco without rot, rot == NULL with nchan > 1; the fmt rules of vit_ofdm_acquire_dev (an unknown
 * format, a scale outside its range; a NULL fmt means float32); nsamples >= 2^60; nout < 0 or nout >
 * vit_resample_out_count(nsamples, p); nchan > 1 with out_stride < nout.  Sample positions stay arbitrary: a CU8 output's
 * first sample may lie at an address that is 2 mod 4.  nout = 0 returns VIT_OK and writes nothing.  Everything is enqueued
 * on `stream` without synchronising; the call needs no buffer of the calling thread. */
int64_t vit_resample_taps(uint32_t L, uint32_t T, double cutoff, float *h_taps);
int64_t vit_resample_out_count(uint64_t nsamples, const vit_resample_params *p);
int vit_iq_resample_dev(const void *d_iq, uint64_t nsamples, const vit_iq_format *fmt /* NULL: float32 */,
                        const vit_resample_params *p, int64_t nout,
                        float *d_out, uint64_t out_stride /* complex samples between channels */, void *stream);

/* From the stream: first acquisition.  What a receiver does first: it has an unaligned stream of samples and must find
 * where the frames start.  One call searches one contiguous stream - float32, or an integer format of "Integer sample
 * formats", which is why the section stands behind it - for the end of each null symbol, the edge where the power comes
 * back, and writes for every frame period one coarse start into a DEVICE table of the kind vit_ofdm_sync_dev reads as
 * in->d_start: samples -> acquire -> sync -> demod -> decode runs without a byte leaving the device.  It is an
 * energy-edge detector and nothing more: no FFT, no correlation, so its starts are right to within about a block and
 * vit_ofdm_sync_dev (W >= B) does the rest.  Like the rest of the front end the result is defined bit for bit. */
typedef struct vit_acq_params {
    uint32_t B;              /* block length, samples: a power of two 8 ... 512 */
    uint32_t null_blocks;    /* Ln: blocks summed in front of a candidate edge, 1 ... 4096 (Ln*B <= the null symbol) */
    uint32_t ref_blocks;     /* Lr: blocks summed behind it, 1 ... 4096 */
    uint32_t period_blocks;  /* Pb: frame period in blocks, >= 1 (mode I at B 32: 6144) */
    float    thr;            /* an edge is accepted when q <= thr; finite, > 0 */
    uint32_t reserved;       /* 0 */
    uint64_t first;          /* the search starts at this sample, <= nsamples; any position */
    int64_t  offset;         /* added to the edge's sample index: e.g. guard + B/2 - backoff, the caller's choice */
} vit_acq_params;
/* Definition.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly this order, never
 * contracted into an FMA.  x: the samples, components from the integer formats by the one-rounding rule of "Integer
 * sample formats"; B, Ln, Lr, Pb, thr, first, offset: the struct's.
 * A. Block power.  nblk = floor((nsamples - first) / B).  Sample i of block j is x[first + j*B + i]:
 *      e[i] = fl( fl(re*re) + fl(im*im) )
 *      p[j] = the tree of adjacent pairs over e[0 ... B-1]: v[i] = fl(v[2i] + v[2i+1]) until one value is left.
 *    d_power, if given, receives p[0 ... nblk-1] and nothing else.
 * B. Windows.  A candidate edge is a j with Ln <= j <= nblk - Lr: the edge lies between blocks j-1 and j.
 *      N[j] = the sum of p[j-Ln+i], i = 0 ... Ln-1, in ascending i, into ONE accumulator that starts at +0: acc = fl(acc + p)
 *      R[j] = the sum of p[j+i],    i = 0 ... Lr-1, in the same way
 *      q[j] = fl(N[j] / R[j]) if R[j] > 0, else +Inf
 * C. Search.  Period k = 0 ... nperiods-1 owns the candidates Ln + k*Pb <= j < Ln + (k+1)*Pb that exist.  j* is the LAST
 *    minimum of q among them: in ascending j, a later j replaces the best when its q is less or equal.  (On a noise-free
 *    stream every j whose front window lies in silence ties at q = 0; the last of them is the block that holds the
 *    edge - the block behind it already has signal in N.)
 * D. Outputs.  d_start_out[k] = first + j* * B + offset if the period has a candidate and q[j*] <= thr, else -1, which
 *    vit_ofdm_sync_dev skips by its own rule.  d_info[4k ...] = {uint32 j* - (Ln + k*Pb), q[j*], N[j*], R[j*]} (optional:
 *    q is the depth of the null, R / (Lr*B) the mean power behind the edge).  A period without candidates gets start -1
 *    and info {0xFFFFFFFF, +Inf, 0, 0}.  Nothing outside the named words is written; no sample at or beyond nsamples and
 *    none in front of `first` is read.
 * The result depends on the samples and the struct alone: never on nperiods (period k has the same words in every call
 * that reaches it), the launch or the device.
 * Domain: every component of a sample is 0 or has a magnitude in [2^-40, 2^12].  Then nothing overflows and no denormal
 * arises anywhere: a product fl(re*re) is 0 or in [2^-80, 2^24], so e is 0 or in [2^-80, 2^25]; all terms are
 * non-negative, so a sum is 0 or at least its smallest nonzero term, 2^-80, and - rounding is monotone and the bounds
 * are powers of two - at most its exact bound: p <= 512 * 2^25 = 2^34, N and R <= 4096 * 2^34 = 2^46.  With R >= 2^-80, q
 * is 0 or lies in [2^-126, 2^126], a normal number.  An all-zero stream is inside the domain: every q is +Inf, j* is the
 * period's last candidate, and every start is -1.  Outside the domain the outputs of the periods that read such samples
 * are unspecified; nothing but the call's output words is written.  The caller keeps first + j* * B + offset inside int64.
 * Arguments as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL d_iq, p or
 * d_start_out; a d_iq that is not aligned as in "Integer sample formats" (8 bytes for float32, 4 for an integer format), a
 * d_start_out that is not 8-byte or a d_info or d_power that is not 4-byte aligned; every range in the struct's comments
 * (thr NaN or Inf among them); a nonzero reserved; first > nsamples; nsamples >= 2^60; nperiods < 0; and the fmt rules of
 * the *_iq_dev calls (an unknown format, a scale outside its range), except that a NULL fmt means float32.  Sample
 * positions stay arbitrary: `first` may be odd, a CU8 block may start at an address that is 2 mod 4.  nperiods = 0 returns
 * VIT_OK and writes nothing, d_power included.  Without d_power the powers live in a buffer of the calling thread, and
 * only those the nperiods periods read are computed.  Everything is enqueued on `stream` without synchronising. */
int vit_ofdm_acquire_dev(const void *d_iq, uint64_t nsamples, const vit_iq_format *fmt /* NULL: float32 */,
                         const vit_acq_params *p, int64_t nperiods,
                         int64_t *d_start_out, uint32_t *d_info /* optional, 4 words per period */,
                         float *d_power /* optional, nblk floats */, void *stream);

/* Transmitter identification.  The null symbol of a transmission frame is silent except for a few carrier PAIRS per
 * transmitter: the transmitter identification information (TII), which tells a receiver which transmitters of a
 * single-frequency network it hears and how strongly.  The used carriers form R repetitions; a repetition has Gp groups
 * of C pairs; a transmitter with main identifier p and sub identifier c switches on pair c in some of the Gp groups -
 * which ones is the pattern of p - and does so identically in every repetition.  One call reads one window of nfft samples
 * per frame - the null symbol - and writes, per group of navg frames, the noise level and per comb c a mask of the groups
 * that stand out of it and their summed power: about 2 + 2C words, with no spectrum in memory.  The pair layout is a
 * caller-supplied DEVICE table (like d_bins and d_prs: the device definition holds and needs no table of the standard);
 * two host helpers below build the standard's tables for mode I.  Like the rest of the front end the result is defined bit
 * for bit. */
typedef struct vit_tii_params {
    uint32_t nfft;      /* power of two 64 ... 8192 */
    uint32_t ngroups;   /* Gp: groups per comb, 1 ... 32 (the standard: 8); a comb's mask is one uint32 */
    uint32_t ncombs;    /* C: pairs per group, >= 1, Gp*C <= 1024 (the standard: 24) */
    uint32_t nrep;      /* R: repetitions across the spectrum, 1 ... 8 (mode I: 4); 2*R*Gp*C <= nfft */
    uint32_t navg;      /* frames summed into one estimate, 1 ... 256 */
    float    thr;       /* a slot is "on" at thr times the noise level; finite, > 0 */
    int64_t  offset;    /* the window starts at the frame's start + offset (mode I, start from vit_ofdm_sync_dev:
                           -(int64_t)sym_stride, i.e. "symbol -1") */
} vit_tii_params;
/* Definition.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly this order, never
 * contracted into an FMA; underflow is gradual, as in vit_ofdm_sync_dev.  in: the struct vit_ofdm_demod_dev takes - the
 * same d_start table, and the d_rot table vit_ofdm_sync_dev wrote.  Gp, C, R, navg, thr, offset: the struct's.
 * ngrp = ceil(nframes / navg); group g owns frames g*navg ... min((g+1)*navg, nframes) - 1.
 * A. Window and spectrum.  Frame t with start s (in->d_start[t], or t*frame_stride) reads samples s + offset + i,
 *    i = 0 ... nfft-1, components from the integer formats by the one-rounding rule of "Integer sample formats".  If
 *    in->d_rot is given they are rotated by step 1 of "From the samples" with n = offset + i: n enters the phase modulo
 *    2^32 as a two's-complement value, so the phase is the one the frame's own symbols continue.  X = the FFT of step 2
 *    of it: the same graph, the same in->d_tw.
 * B. Pair power.  For a table entry k = min(d_pairs[(r*Gp + b)*C + c], nfft-2) (clamped: no entry reads outside the symbol):
 *      e = fl( fl(fl(X[k].re^2) + fl(X[k].im^2)) + fl(fl(X[k+1].re^2) + fl(X[k+1].im^2)) )
 *    f_t[b][c] = the sum of e over r = 0 ... R-1 in ascending r, into ONE accumulator that starts at +0: acc = fl(acc + e).
 * C. Group energy.  E_g[b][c] = the sum of f_t[b][c] over the group's frames in ascending t, in the same way, skipped
 *    frames left out; nused = the number of frames that entered.
 * D. Decision.  noise = the value of rank (Gp*C - 1) / 2 (integer division, 0-based, ascending) among the Gp*C values of
 *    E_g: the lower median.  A selection rounds nothing, and ties do not change the value.
 *      tau = fl(thr * noise)
 *      bit b of mask[c] is set iff E_g[b][c] > 0 and E_g[b][c] >= tau
 *      strength[c] = the sum of the E_g[b][c] whose bit is set, in ascending b, into one accumulator from +0
 * E. Outputs.  d_tii[g*(2 + 2C) ...] = {uint32 nused, noise, mask[0], strength[0], ..., mask[C-1], strength[C-1]}, floats as
 *    their bit patterns.  d_energy, if given, receives E_g[b][c] at (g*Gp + b)*C + c.  A group with nused = 0 gets zeros
 *    throughout.  Nothing else is written; no sample outside the windows is read.
 * The result depends on the samples, the tables and the struct alone: never on nframes beyond the group's own frames
 * (group g has the same words in every call that holds all its frames), the launch or the device.
 * Domain: the samples' domain of "From the samples" with magnitudes up to 2^12.  Then nothing overflows: the rotation
 * keeps a magnitude (up to sqrt 2 per component), a spectrum component is a sum of nfft <= 2^13 such terms, at most
 * 2^13 * 2^12 * sqrt 2 < 2^26; its square is under 2^52, e under 2^54, and the sums have at most R * navg = 8 * 256 terms
 * (strength: Gp = 32 more): under 2^54 * 2^11 * 2^5 = 2^70.  tau = fl(thr * noise) may overflow to +Inf for a thr near
 * FLT_MAX: then no bit is set.  All-zero windows are inside the domain: noise 0, every mask 0 (E > 0 fails).  Outside the
 * domain the outputs of the groups that read such samples are unspecified; nothing but the call's output words is written.
 * Skip rule: with in->d_start given, a frame with a negative start (the -1 of vit_ofdm_acquire_dev and
 * vit_ofdm_sync_dev) is skipped, and so is a frame whose window is not inside [0, nsamples).  Without the table such a
 * frame is VIT_ERR_ARG.
 * Arguments as the other *_dev calls: VIT_ERR_NO_DEVICE first; VIT_ERR_ARG (with vit_last_error()) for a NULL in, p, d_iq,
 * d_tw, d_pairs or d_tii; a d_iq that is not aligned as in "Integer sample formats" (8 bytes for float32, 4 for an integer
 * format), a d_tw, d_nco, d_start or d_rot that is not 8-byte aligned, a d_pairs that is not 2-byte or a d_tii or d_energy
 * that is not 4-byte aligned; every range in the struct's comments (thr NaN or Inf among them); d_rot without d_nco or with
 * nco_bits outside 1 ... 20; the fmt rules of the *_iq_dev calls, except that a NULL fmt means float32; nframes < 0 or
 * above 2^31 - 1.
 * in->sym_stride is not read.  nframes = 0 returns VIT_OK and writes nothing.  The per-frame pair powers live in a buffer
 * of the calling thread.  Everything is enqueued on `stream` without synchronising.
 *
 * The two host helpers hold what the standard's clause on TII says for mode I, as far as it is needed to use the call;
 * the device definition depends on neither.  Both need no GPU.
 *   vit_tii_pair_bins(1, h_pairs) writes the 768 entries of the d_pairs table for nfft = 2048, R = 4, Gp = 8, C = 24 and
 *     returns 768: entry (r*8 + b)*24 + c is the FFT bin of carrier k0 = base[r] + 2c + 48b, base = {-768, -384, 1, 385},
 *     a carrier k < 0 lying at bin 2048 + k; the pair is carriers k0 and k0 + 1.  Any other mode (II - IV were withdrawn
 *     from the standard) or a NULL pointer returns -1.
 *   vit_tii_main_id(mask): bit b of mask is group b, as in d_tii.  The standard's pattern word of a main identifier puts
 *     group 0 in the MOST significant of its 8 bits; p is the rank of that word among the 70 eight-bit words with four
 *     ones, in ascending numeric order: p = 0 is 0x0F, p = 1 is 0x17, ..., p = 69 is 0xF0.  So mask 0xF0 (groups 4 ... 7)
 *     is p = 0.  Returns 0 ... 69, or -1 if the mask has not exactly four bits set or is above 255 (two transmitters
 *     sharing a comb give the union of their patterns: the caller splits it by strength or over time). */
int vit_ofdm_tii_dev(const vit_iq_input *in, const vit_iq_format *fmt /* NULL: float32 */, const vit_tii_params *p,
                     const uint16_t *d_pairs /* DEVICE, R*Gp*C lower bins, index (r*Gp + b)*C + c */,
                     int64_t nframes, uint32_t *d_tii /* ngrp * (2 + 2*C) words */,
                     float *d_energy /* optional, ngrp * Gp*C floats */, void *stream);
int64_t vit_tii_pair_bins(uint32_t mode, uint16_t *h_pairs);   /* host only: mode 1 -> 768 entries; else -1 */
int     vit_tii_main_id(uint32_t mask);                        /* host only: 0 ... 69, or -1 if popcount != 4 or mask > 255 */

/* Channel-state weighting: a second soft-decision rule.  The definition of vit_ofdm_demap_dev scales every carrier by its
 * own |re| + |im|, so a carrier in a fading notch reaches the decoder with the confidence of the strongest one.  The
 * per-symbol rule scales all K carriers of an OFDM symbol by one value, taken from the mean of |re| + |im| over the
 * symbol: a carrier's soft value then grows with its strength (|H|^2 for differential detection), which is the weight a
 * Viterbi decoder wants.  The existing calls, their bytes and their kernels are untouched; the rule is a HOST struct read
 * during the call. */
#define VIT_SOFT_PER_CARRIER 0   /* the definition of vit_ofdm_demap_dev */
#define VIT_SOFT_PER_SYMBOL  1
typedef struct vit_soft_rule {
    uint32_t rule;        /* VIT_SOFT_* */
    float    gain;        /* PER_CARRIER: 0 < gain <= 65536;  PER_SYMBOL: 2^-24 <= gain <= 65536 */
} vit_soft_rule;
/* Definition of VIT_SOFT_PER_SYMBOL.  Every operation is one IEEE binary32 operation, rounded to nearest-even, in exactly
 * this order, never contracted into an FMA.  Per data symbol:
 * 1. re, im and nrm of every n = 0 ... K-1 exactly as in vit_ofdm_demap_dev.
 *      v[n] = nrm[n]  if 2^-64 <= nrm[n] <= FLT_MAX,  else +0          (no signal, NaN, Inf: the carrier is an erasure)
 * 2. The symbol's level S = the sum of v in a grouping that depends on nfft and K alone - never on nframes, the launch or
 *    the device - in the shape of the long sums of "From the coarse start":
 *      groups        q[g] = fl( fl(v[4g] + v[4g+1]) + fl(v[4g+2] + v[4g+3]) )  for g < ceil(K/4); a v[n] with n >= K is +0
 *      accumulators  A = max(64, nfft/8) of them:  acc[i] = q[i], then acc[i] = fl(acc[i] + q[i+A]), then + q[i+2A] ... in
 *                    this order while the group exists (K <= nfft: at most two); acc[i] = +0 for i >= ceil(K/4)
 *      tree          the accumulators meet in the tree of adjacent pairs: u[i] = fl(u[2i] + u[2i+1]) until one is left
 *    All terms are non-negative: an overflow gives +Inf, never NaN.
 * 3. If not (2^-64 <= S <= 2^96): all 2K bytes of the symbol are 128 (no signal at all, or a level beyond any receiver's).
 * 4. Otherwise  s = fl( fl(gain * fl(K)) / S )                          fl(K) is exact
 *      a carrier with v[n] = +0:  out[n] = out[n+K] = 128
 *      every other carrier:       out[n]   = clamp(128 - rint(fl(re*s)), 0, 255)
 *                                 out[n+K] = clamp(128 - rint(fl(im*s)), 0, 255)      rint: ties to even
 *    An ideal constellation point on a carrier of the symbol's mean strength gives 128 -/+ gain/2; a carrier of twice the
 *    mean amplitude four times that excursion, up to the clamp.  Gains of 64 ... 128 suit the decoders here (INTEGRATION.md
 *    2i); the per-carrier rule's 254 would clamp every carrier above the mean.
 * The bounds, checked: gain*K lies in [2^-24, 2^29] and S in [2^-64, 2^96], so s lies in [2^-120, 2^93] and is a normal
 * number.  Every term of S is 0 or at least 2^-64, so no partial sum is denormal.  re and im of a carrier that is no
 * erasure are finite (nrm <= FLT_MAX).  fl(re*s) may be denormal or, with flushing, 0 - then |re*s| < 2^-126 and rint
 * gives 0 either way; a denormal re times s <= 2^93 stays under 2^-33 and rounds to 0 either way; an overflow of re*s
 * gives +-Inf and clamps.  So no byte depends on how denormals are handled, as in the per-carrier rule.
 * No run of symbols influences another symbol: a symbol's bytes and level are the same in every launch.
 *
 * The two calls: vit_ofdm_demap_soft_dev is vit_ofdm_demap_dev, and vit_ofdm_demod_soft_dev is vit_ofdm_demod_iq_dev (fmt
 * NULL: float32 samples, vit_ofdm_demod_dev), with `soft` in the place of gain.  Every argument that soft does not replace
 * means what it means there: destinations, skipped frames, guarantees and argument rules.  With VIT_SOFT_PER_CARRIER the
 * call dispatches to the existing kernels and gives the existing call's bytes; d_level must then be NULL.
 * d_level: optional DEVICE table of nframes * (nsyms-1) floats, 4-byte aligned.  Word t*(nsyms-1) + s receives S of data
 * symbol s of frame t, for the symbols the call demaps (FIC only, MSC only or both); the other words, and all words of a
 * frame skipped through d_start, keep their old value.  It is the caller's signal-level and lock input (S / K is the mean
 * of |re| + |im|, about sqrt 2 times the mean carrier power), and it makes the summation order observable.
 * In addition VIT_ERR_ARG (with vit_last_error()) for a NULL soft, a rule other than the two, d_level with
 * VIT_SOFT_PER_CARRIER, a misaligned d_level, and with VIT_SOFT_PER_SYMBOL a gain outside [2^-24, 65536] (NaN included). */
int vit_ofdm_demap_soft_dev(const float *d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t *d_bins,
                            const vit_ofdm_shape *shape, const vit_soft_rule *soft, int64_t nframes, uint8_t *d_fic,
                            const vit_cif_ring *ring, uint64_t col, float *d_level, void *stream);
int vit_ofdm_demod_soft_dev(const vit_iq_input *in, const vit_iq_format *fmt /* NULL: float32 */,
                            const uint16_t *d_bins, const vit_ofdm_shape *shape, const vit_soft_rule *soft,
                            int64_t nframes, uint8_t *d_fic, const vit_cif_ring *ring, uint64_t col,
                            float *d_level, void *stream);

/* Kernel selection (the analogue of the reference's dispatcher, setupdll.cpp:195-270):
 *   0 = auto: launches of up to 2048 frames (they cannot fill the chip) take the latency kernel - one
 *       frame per wavefront, ~20 us per FIC frame -, larger ones the packed throughput kernel;
 *   1 = wave-per-frame cross-check kernel, 2 = packed 4-frames-per-wave kernel, 3 = latency kernel,
 *   4 = packed 8-frames-per-wave kernel (frames <= 778 bits; an experiment kept for comparison: fewer instructions per
 *       frame, slower - see csrc/vit_pk8.hip).
 * Returns the old value.  Affects later vit_decode_* / deconvolve calls of the whole process. */
int vit_set_kernel(int which);

/* Renormalisation comparator of the decoder (process-wide, affects later vit_decode_* / deconvolve calls).
 * The reference exists in two build configurations that differ in ONE comparison on the hot path:
 *   1 (default): renormalise when the metric of state 0 is >= 150 -- the MASM decoders, decon_avx2.asm:97,114
 *                `cmp sil,150 ; jb mainloop` (also decon_avx.asm:142, decon_ssse3.asm:163,
 *                decon_sse2_lut32.asm:173; configuration Rel_asm, the one the reference's README tells users to
 *                build (README.md:50-52): what an installed viterbi.dll runs);
 *   0          : renormalise when it is                    >  150 -- the C decoders, deconvolve.cpp:399,408
 *                (configuration Rel_cpp, the one that can be compiled and run outside Windows; bench.py selects it
 *                because its timed CPU baseline, this repo's AVX2 port, implements it).
 * The two give identical output on soft-decision input at any usable SNR and DIFFERENT output on hard-decision
 * (0/255) input from a poor channel, where path metrics reach the 0 and 255 clamps (tests/test_gpu_parity.py:
 * test_renorm_ge_mode).  Environment variable VITERBI_AMD_RENORM_GE=0/1 selects the mode at start-up for a host that
 * only binds the five reference exports.  Returns the previous value.  (Until round 3 the default was 0.) */
int vit_set_renorm_ge(int on);

/* ------------------------------------------------------------------------ *
 * Part 3 -- several GPUs behind one call (BASELINE.json configs[3], SURVEY 8e;
 * not in the reference, whose only concurrency is caller threads, README.md:56)
 * ------------------------------------------------------------------------ */

/* ONE host process, ndev gfx950 devices (HIP ordinals in devices[], distinct; devices[0] is the "root").
 * nframes equal-length frames in the device format live on the root (d_symbols_u8), the decoded bytes
 * are wanted there too (d_decoded).  The stream is cut into chunks of
 *     root_frames + (ndev-1) * chunk_frames
 * consecutive frames; of every chunk the root decodes the first root_frames itself and devices[i]
 * (i >= 1) the i-th block of chunk_frames frames: round-robin at block granularity, so each block is
 * a contiguous slice that RCCL sends from / receives into place (ncclSend/ncclRecv over xGMI, one
 * ncclGroupStart/End per pipeline step, librccl dlopen'ed on first use).  Block k+1 travels while
 * block k is being decoded and the decoded bytes of block k-1 come back (double buffers per device).
 *   root_frames : -1 = chunk_frames; 0 = the root only distributes (ndev > 1); larger values give the
 *                 root a bigger share (its peers are fed through one xGMI link each)
 *   stream      : the root-device stream that produced d_symbols_u8 (NULL = default stream); the
 *                 transfers start behind it
 *   flags       : VIT_MULTI_LOOPBACK adds one more rank ON THE ROOT DEVICE that is fed through RCCL
 *                 like a remote peer (self send/recv) - a self-test of the pipeline on a one-GPU box
 * SYNCHRONOUS: returns when every byte of d_decoded is in place.  One call at a time per process
 * (internal mutex); streams, communicators and buffers are cached between calls with the same devices.
 * The caller's current device is restored.  ndev == 1 without the flag needs no RCCL. */
#define VIT_MULTI_LOOPBACK 0x1u
int vit_decode_stream_multi(const uint8_t *d_symbols_u8, uint8_t *d_decoded, uint32_t framebits,
                            int64_t nframes, const int *devices, int ndev, int64_t chunk_frames,
                            int64_t root_frames, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VITERBI_AMD_H */
