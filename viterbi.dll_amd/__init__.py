"""viterbi.dll_amd -- Python host mirror of the drop-in C ABI (libviterbi.so).

The product is the shared library built from csrc/ (hand-written HIP kernels for
gfx950 behind the reference's exported C functions, include/viterbi_amd.h).  This
module is the thin ctypes binding used by tests and bench.py; names and argument
meaning follow the reference exports (viterbi.def:4-8): ``deconvolve``,
``RScheckSuperframe``, ``initialize``, ``GetCPUCaps``, ``WakeUpYMM`` -- plus the
batched device-resident extension.  There is no CPU fallback here: if the
library is missing, or no gfx950 device is present, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH_DEFAULT = os.path.join(_HERE, "libviterbi.so")
LIB_PATH = os.environ.get("VITERBI_AMD_LIB") or LIB_PATH_DEFAULT  # env: kernel experiments, the tests' -DVIT_DIAG_SPEC build
MAX_FRAMEBITS = 9216
TAIL = 6

EXPORTS = [
    "deconvolve", "initialize", "RScheckSuperframe", "RSCheckSuperframe", "GetCPUCaps", "WakeUpYMM",
    "vit_last_error", "vit_device_count", "vit_set_kernel", "vit_set_renorm_ge", "vit_set_batch_window_us", "vit_set_batch_min_callers", "vit_set_batch_depth", "vit_set_batch_spin_cpus",
    "vit_decode_batch_dev",
    "vit_decode_batch_dev_u32", "vit_decode_varlen_dev", "vit_decode_varlen_dev_checked", "vit_pack_symbols_dev", "vit_sort_descs",
    "vit_decode_batch_host", "vit_rs_batch_dev", "vit_rs_batch_host", "vit_dabplus_superframes_dev",
    "vit_punctured_length", "vit_decode_punctured_dev", "vit_decode_punctured_varlen_dev",
    "vit_energy_dispersal_prbs", "vit_energy_dispersal_dev", "vit_energy_dispersal_varlen_dev", "vit_fib_crc_dev",
    "vit_decode_fic_dev", "vit_dabplus_punctured_superframes_dev",
    "vit_dabplus_aus_dev", "vit_dabplus_aus_host", "vit_fire_code_dev",
    "vit_time_deinterleave_dev", "vit_decode_punctured_ti_dev", "vit_dabplus_ti_superframes_dev",
    "vit_ensemble_layout", "vit_rs_table_dev", "vit_dabplus_aus_table_dev", "vit_ensemble_dev",
    "vit_freq_interleave_bins", "vit_ofdm_demap_dev",
    "vit_fft_twiddles", "vit_nco_table", "vit_ofdm_fft_dev", "vit_ofdm_demod_dev", "vit_ofdm_sync_dev",
    "vit_ofdm_fft_iq_dev", "vit_ofdm_demod_iq_dev", "vit_ofdm_sync_iq_dev", "vit_iq_convert_dev",
    "vit_ofdm_demap_soft_dev", "vit_ofdm_demod_soft_dev", "vit_ofdm_acquire_dev",
    "vit_ofdm_tii_dev", "vit_tii_pair_bins", "vit_tii_main_id",
    "vit_resample_taps", "vit_resample_out_count", "vit_iq_resample_dev",
    "vit_packet_fec_sync_dev", "vit_packet_fec_count", "vit_packet_fec_dev", "vit_packet_fec_frame_host", "vit_packets_dev",
    "vit_data_groups_dev", "vit_data_groups_host", "vit_packet_table_layout", "vit_packet_table_dev",
    "vit_data_groups_table_layout", "vit_data_groups_table_dev",
    "vit_mci_fibs_dev", "vit_mci_fibs_host", "vit_eep_profile", "vit_mci_ens_table",
    "vit_mci_dir_dev", "vit_mci_dir_host", "vit_mci_dir_ens_table", "vit_mci_pkt_table",
    "vit_decode_stream_multi",
]
MULTI_LOOPBACK = 0x1


class ViterbiError(RuntimeError):
    pass


class FrameDesc(C.Structure):
    """vit_frame_desc of include/viterbi_amd.h"""
    _fields_ = [("sym_offset", C.c_uint64), ("out_offset", C.c_uint64),
                ("framebits", C.c_uint32), ("reserved", C.c_uint32)]


DESC_DTYPE = np.dtype([("sym_offset", "<u8"), ("out_offset", "<u8"), ("framebits", "<u4"), ("reserved", "<u4")])

# vit_au_table of include/viterbi_amd.h: one record per DAB+ superframe
AU_DTYPE = np.dtype([("status", "u1"), ("num_aus", "u1"), ("param", "u1"), ("crc_ok", "u1"), ("au_start", "<u2", (7,)),
                     ("fire_ok", "u1"), ("reserved", "u1")])
AU_OK, AU_RS_FAILED, AU_BAD_HEADER = 0, 1, 2

# packet mode (include/viterbi_amd.h): vit_fec_rec per FEC frame, vit_packet_rec per 24-byte slot
FEC_REC_DTYPE = np.dtype([("nerr", "i1", (12,)), ("hdr_ok", "<u2"), ("status", "u1"), ("reserved", "u1")])
PACKET_REC_DTYPE = np.dtype([("kind", "u1"), ("crc_ok", "u1"), ("nslots", "u1"), ("flags", "u1"), ("address", "<u2"),
                             ("useful", "u1"), ("reserved", "u1")])
PKT_CONT, PKT_DATA, PKT_PADDING, PKT_FEC, PKT_OVERRUN = 0, 1, 2, 3, 4
PKT_SLOT, FEC_FRAME_SLOTS, FEC_FRAME_BYTES = 24, 103, 2472
PKT_LAST, PKT_FIRST = 4, 8  # vit_packet_rec.flags
# packet mode over a table of streams: vit_pkt_stream per entry, vit_pkt_layout, vit_pkt_stream_rec per stream
PKT_MAX_STREAMS = 64
PKT_FEC_NONE, PKT_FEC_PHASE, PKT_FEC_SEARCH = 0, 1, 2
PKT_NO_PHASE = 0xFFFFFFFF
PKT_STREAM_DTYPE = np.dtype([("offset", "<u8"), ("framebytes", "<u4"), ("nframes", "<u4"), ("fec", "<u4"), ("phase", "<u4"),
                             ("min_score", "<u4"), ("reserved", "<u4")])
PKT_LAYOUT_DTYPE = np.dtype([("rec_index", "<u8", (PKT_MAX_STREAMS,)), ("fec_index", "<u8", (PKT_MAX_STREAMS,)), ("nrec", "<u8"),
                             ("nfecrec", "<u8"), ("bytes_end", "<u8")])
PKT_STREAM_REC_DTYPE = np.dtype([("phase", "<u4"), ("score", "<u4"), ("runner_up", "<u4"), ("nfec", "<u4")])
# MSC data groups: vit_dgroup_rec per group, vit_dgroup_summary per call
DGROUP_REC_DTYPE = np.dtype([("first_slot", "<u4"), ("last_slot", "<u4"), ("npackets", "<u4"), ("offset", "<u4"), ("length", "<u4"),
                             ("address", "<u2"), ("segment", "<u2"), ("transport_id", "<u2"), ("payload_offset", "<u2"),
                             ("type", "u1"), ("cont_rep", "u1"), ("flags", "u1"), ("command", "u1")])
DGROUP_SUM_DTYPE = np.dtype([("ngroups", "<u4"), ("nwritten", "<u4"), ("data_bytes", "<u4"), ("open_from", "<u4"), ("n_used", "<u4"),
                             ("n_dropped", "<u4"), ("n_unusable", "<u4"), ("reserved", "<u4")])
DGF_WELLFORMED, DGF_CRCF, DGF_CRC_OK, DGF_SEG, DGF_UA, DGF_TIDF, DGF_EXT = 1, 2, 4, 8, 16, 32, 64
DGROUP_MAX_SLOTS = 1 << 24
# the slot counts at which the kernels of csrc/vit_dgroup.hip change their partition (TILE, CHUNK, NUM_BLOCK, GATHER_STEP
# there): the link pass's tile and the chunk of one workgroup, the block of the prefix sum, the slots a gathering wavefront
# takes per step.  Every group is gathered by one wavefront: there is no wavefront/workgroup threshold.
DGROUP_GEOMETRY = {"link_tile": 1024, "link_chunk": 16384, "number_block": 4096, "gather_step": 64}
# data groups over a table of streams: vit_dg_stream per entry, vit_dg_layout
DG_MAX_STREAMS = 64
DG_STREAM_DTYPE = np.dtype([("offset", "<u8"), ("rec_index", "<u8"), ("nslots", "<u4"), ("max_groups", "<u4"), ("data_capacity", "<u4"),
                            ("records_only", "<u4")])
DG_LAYOUT_DTYPE = np.dtype([("dg_index", "<u8", (DG_MAX_STREAMS,)), ("data_offset", "<u8", (DG_MAX_STREAMS,)), ("ndg", "<u8"),
                            ("data_bytes", "<u8"), ("bytes_end", "<u8"), ("rec_end", "<u8")])
# the sizes at which the kernels of csrc/vit_ofdm_acq.hip change their partition (TILE_CHUNKS and the chunk's 16 bytes,
# SEARCH_TILE, WINDOW_MAX there): the 16-byte chunks a wavefront of the power kernel takes per trip, the candidates the
# search holds in LDS at once, the longest window the LDS is sized for
ACQ_GEOMETRY = {"chunk_bytes": 16, "tile_chunks": 256, "search_tile": 2048, "window_max": 4096}
# and of csrc/vit_ofdm_tii.hip (GROUP_TPB, SLOTS_MAX there, and the argument rules' caps): the threads of the group kernel,
# whose three loops step by that many slots or combs, the slots its LDS holds, and the most groups, frames per estimate
# and repetitions the call takes
TII_GEOMETRY = {"group_threads": 256, "slots_max": 1024, "groups_max": 32, "navg_max": 256, "nrep_max": 8}

# multiplex configuration (include/viterbi_amd.h): vit_mci_subch per (group, SubChId), vit_mci_group per group
MCI_SUBCH_DTYPE = np.dtype([("org", "<u4"), ("comp", "<u4"), ("sid", "<u4"), ("n_org", "<u2"), ("n_org_other", "<u2"),
                            ("n_comp", "<u2"), ("n_comp_other", "<u2")])
MCI_GROUP_DTYPE = np.dtype([("eid", "<u2"), ("cif", "<u2"), ("flags", "u1"), ("reserved", "u1"), ("nfib_used", "<u2"),
                            ("nfib_malformed", "<u2"), ("n_ens_other", "<u2"), ("n_next", "<u2"), ("reserved2", "<u2")])
MCI_USED, MCI_MALFORMED, MCI_FIG00, MCI_FIG01, MCI_FIG02 = 1, 2, 4, 8, 16
MCI_MAX_G = 4096
# service directory: vit_mci_service and vit_mci_pktcomp per (group, record), vit_mci_dir per group
DIR_MAX = 64
MCI_SERVICE_DTYPE = np.dtype([("sid", "<u4"), ("label", "u1", (16,)), ("chars", "<u2"), ("flags", "u1"), ("count", "u1"),
                              ("n_label", "<u2"), ("n_label_other", "<u2"), ("n_listed", "<u2"), ("n_listed_other", "<u2")])
MCI_PKTCOMP_DTYPE = np.dtype([("scid", "<u2"), ("flags", "<u2"), ("loc", "<u4"), ("sid", "<u4"), ("n_loc", "<u2"),
                              ("n_loc_other", "<u2"), ("n_comp", "<u2"), ("n_comp_other", "<u2")])
MCI_DIR_DTYPE = np.dtype([("eid", "<u2"), ("chars", "<u2"), ("label", "u1", (16,)), ("flags", "u1"), ("charset", "u1"),
                          ("n_label", "<u2"), ("n_label_other", "<u2"), ("nsvc", "<u2"), ("npkt", "<u2"), ("nfib_used", "<u2"),
                          ("nfib_malformed", "<u2"), ("n_next", "<u2"), ("reserved", "<u2", (2,))])
MCI_DIR_USED, MCI_DIR_MALFORMED, MCI_DIR_FIG02, MCI_DIR_FIG03, MCI_DIR_FIG1 = 1, 2, 4, 8, 16

# vit_ens_subch / vit_ens_layout of include/viterbi_amd.h: one entry per sub-channel of an ensemble, and where its blocks lie
ENS_MAX_SUBCH = 64
ENS_SUBCH_DTYPE = np.dtype([("col", "<u4"), ("profile", "<u4"), ("framebits", "<u4"), ("RSDims", "<u4"), ("phase", "<u4"),
                            ("nframes", "<u4"), ("nsym", "<u4"), ("reserved", "<u4")])
ENS_LAYOUT_DTYPE = np.dtype([("work_offset", "<u8", (ENS_MAX_SUBCH,)), ("rs_offset", "<u8", (ENS_MAX_SUBCH,)),
                             ("rec_index", "<u8", (ENS_MAX_SUBCH,)), ("work_bytes", "<u8"), ("rs_bytes", "<u8"), ("nrec", "<u8"),
                             ("rows_needed", "<u4"), ("max_framebits", "<u4")])

PUNCT_MAX_SEGS = 8


class PunctSeg(C.Structure):
    """vit_punct_seg of include/viterbi_amd.h"""
    _fields_ = [("steps", C.c_uint32), ("keep", C.c_uint32)]


class PunctProfile(C.Structure):
    """vit_punct_profile of include/viterbi_amd.h (68 bytes; bytes(profile) is its device image)"""
    _fields_ = [("nsegs", C.c_uint32), ("seg", PunctSeg * PUNCT_MAX_SEGS)]


class CifRing(C.Structure):
    """vit_cif_ring of include/viterbi_amd.h: a ring of CIF rows on the device"""
    _fields_ = [("d_base", C.c_void_p), ("row_bytes", C.c_uint64), ("nrows", C.c_uint32), ("first_row", C.c_uint32)]


class OfdmShape(C.Structure):
    """vit_ofdm_shape of include/viterbi_amd.h: OfdmShape(nfft, ncarriers, nsyms, fic_syms, cifs)"""
    _fields_ = [("nfft", C.c_uint32), ("ncarriers", C.c_uint32), ("nsyms", C.c_uint32), ("fic_syms", C.c_uint32),
                ("cifs", C.c_uint32)]


class IqInput(C.Structure):
    """vit_iq_input of include/viterbi_amd.h: baseband samples on the device and the tables of the front end"""
    _fields_ = [("d_iq", C.c_void_p), ("nsamples", C.c_uint64), ("sym_stride", C.c_uint64), ("frame_stride", C.c_uint64),
                ("d_start", C.c_void_p), ("d_tw", C.c_void_p), ("d_nco", C.c_void_p), ("nco_bits", C.c_uint32),
                ("d_rot", C.c_void_p)]


class IqFormat(C.Structure):
    """vit_iq_format of include/viterbi_amd.h: IqFormat(format, scale)"""
    _fields_ = [("format", C.c_uint32), ("scale", C.c_float)]


# the sample formats of include/viterbi_amd.h (VIT_IQ_*) and the tensor types that hold them
IQ_F32, IQ_CU8, IQ_CS8, IQ_CS16 = 0, 1, 2, 3
_IQ_DTYPES = {IQ_CU8: "torch.uint8", IQ_CS8: "torch.int8", IQ_CS16: "torch.int16"}


class SoftRule(C.Structure):
    """vit_soft_rule of include/viterbi_amd.h: SoftRule(rule, gain)"""
    _fields_ = [("rule", C.c_uint32), ("gain", C.c_float)]


# the soft-decision rules of include/viterbi_amd.h (VIT_SOFT_*)
SOFT_PER_CARRIER, SOFT_PER_SYMBOL = 0, 1


class SyncParams(C.Structure):
    """vit_sync_params of include/viterbi_amd.h: SyncParams(nfft, nsyms, cp_symbols, W, M, thr, backoff, first_start)"""
    _fields_ = [("nfft", C.c_uint32), ("nsyms", C.c_uint32), ("cp_symbols", C.c_uint32), ("W", C.c_uint32), ("M", C.c_uint32),
                ("thr", C.c_float), ("backoff", C.c_int32), ("first_start", C.c_int64)]


class AcqParams(C.Structure):
    """vit_acq_params of include/viterbi_amd.h: AcqParams(B, null_blocks, ref_blocks, period_blocks, thr, reserved, first,
    offset)"""
    _fields_ = [("B", C.c_uint32), ("null_blocks", C.c_uint32), ("ref_blocks", C.c_uint32), ("period_blocks", C.c_uint32),
                ("thr", C.c_float), ("reserved", C.c_uint32), ("first", C.c_uint64), ("offset", C.c_int64)]


class TiiParams(C.Structure):
    """vit_tii_params of include/viterbi_amd.h: TiiParams(nfft, ngroups, ncombs, nrep, navg, thr, offset)"""
    _fields_ = [("nfft", C.c_uint32), ("ngroups", C.c_uint32), ("ncombs", C.c_uint32), ("nrep", C.c_uint32),
                ("navg", C.c_uint32), ("thr", C.c_float), ("offset", C.c_int64)]


class ResampleParams(C.Structure):
    """vit_resample_params of include/viterbi_amd.h: ResampleParams(L, M, T, nchan, pos0, d_taps, d_nco, nco_bits, reserved,
    rot)"""
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("T", C.c_uint32), ("nchan", C.c_uint32), ("pos0", C.c_uint64),
                ("d_taps", C.c_void_p), ("d_nco", C.c_void_p), ("nco_bits", C.c_uint32), ("reserved", C.c_uint32),
                ("rot", C.c_void_p)]


RESAMPLE_MAX_CHAN = 16

# the four transmission modes of EN 300 401 as shapes (examples: the library compiles in no table of modes)
OFDM_MODES = {1: (2048, 1536, 76, 3, 4), 2: (512, 384, 76, 3, 1), 3: (256, 192, 153, 8, 1), 4: (1024, 768, 76, 3, 2)}

_lib = None


def build(force=False, extra=(), out=None):
    from importlib import util as _u
    spec = _u.spec_from_file_location("_vit_build", os.path.join(_HERE, "build.py"))
    mod = _u.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(force=force, extra=extra, out=out)


def lib():
    """Load libviterbi.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ViterbiError("libviterbi.so not built: run `python __graft_entry__.py build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.deconvolve.argtypes = [C.c_uint, vp, C.c_int, vp]
        L.deconvolve.restype = C.c_int
        L.initialize.restype = C.c_ubyte
        L.RScheckSuperframe.argtypes = [vp, C.c_int, C.c_uint, vp]
        L.RSCheckSuperframe.argtypes = [vp, C.c_int, C.c_uint, vp]
        L.GetCPUCaps.restype = C.c_int
        L.WakeUpYMM.restype = None
        L.vit_last_error.restype = C.c_char_p
        L.vit_set_kernel.argtypes = [C.c_int]
        L.vit_set_renorm_ge.argtypes = [C.c_int]
        L.vit_set_batch_window_us.argtypes = [C.c_int]
        L.vit_set_batch_min_callers.argtypes = [C.c_int]
        L.vit_set_batch_depth.argtypes = [C.c_int]
        L.vit_set_batch_spin_cpus.argtypes = [C.c_int]
        L.vit_decode_batch_dev.argtypes = [vp, vp, C.c_uint32, C.c_int64, vp]
        L.vit_decode_batch_dev_u32.argtypes = [vp, vp, C.c_uint32, C.c_int64, vp]
        L.vit_decode_varlen_dev.argtypes = [vp, vp, vp, C.c_int64, C.c_uint32, vp]
        L.vit_decode_varlen_dev_checked.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_int64, C.c_uint32, vp]
        L.vit_pack_symbols_dev.argtypes = [vp, vp, C.c_int64, vp]
        L.vit_sort_descs.argtypes = [vp, C.c_int64]
        L.vit_sort_descs.restype = None
        L.vit_decode_batch_host.argtypes = [vp, vp, C.c_uint32, C.c_int64]
        L.vit_rs_batch_dev.argtypes = [vp, vp, vp, C.c_uint32, C.c_int64, vp]
        L.vit_rs_batch_host.argtypes = [vp, vp, vp, C.c_uint32, C.c_int64]
        L.vit_dabplus_superframes_dev.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_int64, vp]
        L.vit_decode_stream_multi.argtypes = [vp, vp, C.c_uint32, C.c_int64, vp, C.c_int, C.c_int64, C.c_int64, C.c_uint, vp]
        L.vit_punctured_length.argtypes = [C.POINTER(PunctProfile), C.c_uint32]
        L.vit_punctured_length.restype = C.c_int64
        L.vit_decode_punctured_dev.argtypes = [vp, vp, C.c_uint32, C.c_int64, C.POINTER(PunctProfile), C.c_uint8, vp]
        L.vit_decode_punctured_varlen_dev.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_int64, C.c_uint32, vp,
                                                      C.c_uint32, C.c_uint8, vp]
        L.vit_energy_dispersal_prbs.argtypes = [vp, C.c_uint32]
        L.vit_energy_dispersal_prbs.restype = C.c_int64
        L.vit_energy_dispersal_dev.argtypes = [vp, C.c_uint32, C.c_int64, vp]
        L.vit_energy_dispersal_varlen_dev.argtypes = [vp, C.c_uint64, vp, C.c_int64, vp]
        L.vit_fib_crc_dev.argtypes = [vp, C.c_int64, vp, vp]
        L.vit_decode_fic_dev.argtypes = [vp, vp, vp, C.c_uint32, C.c_int64, C.POINTER(PunctProfile), C.c_uint8, vp]
        L.vit_dabplus_punctured_superframes_dev.argtypes = [vp, C.POINTER(PunctProfile), C.c_uint8, vp, vp, vp, vp,
                                                            C.c_uint32, C.c_int64, vp]
        L.vit_dabplus_aus_dev.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_int64, vp, vp, vp]
        L.vit_dabplus_aus_host.argtypes = [vp, C.c_uint32, vp]
        L.vit_fire_code_dev.argtypes = [vp, C.c_uint64, C.c_int64, vp, vp]
        pr, pp = C.POINTER(CifRing), C.POINTER(PunctProfile)
        L.vit_time_deinterleave_dev.argtypes = [pr, C.c_uint64, C.c_uint32, vp, C.c_int64, vp]
        L.vit_decode_punctured_ti_dev.argtypes = [pr, C.c_uint64, vp, C.c_uint32, C.c_int64, pp, C.c_uint8, vp]
        L.vit_dabplus_ti_superframes_dev.argtypes = [pr, C.c_uint64, pp, C.c_uint8, vp, vp, vp, vp, C.c_uint32, C.c_int64, vp]
        L.vit_ensemble_layout.argtypes = [vp, C.c_uint32, vp]
        L.vit_rs_table_dev.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
        L.vit_dabplus_aus_table_dev.argtypes = [vp, C.c_int, vp, C.c_uint32, vp, vp, vp]
        L.vit_ensemble_dev.argtypes = [pr, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_uint8, vp, vp, vp, vp, vp, vp]
        L.vit_freq_interleave_bins.argtypes = [C.c_uint32, vp]
        L.vit_freq_interleave_bins.restype = C.c_int64
        L.vit_ofdm_demap_dev.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.POINTER(OfdmShape), C.c_float, C.c_int64, vp, pr,
                                         C.c_uint64, vp]
        pi = C.POINTER(IqInput)
        L.vit_fft_twiddles.argtypes = [C.c_uint32, vp]
        L.vit_fft_twiddles.restype = C.c_int64
        L.vit_nco_table.argtypes = [C.c_uint32, vp]
        L.vit_nco_table.restype = C.c_int64
        L.vit_ofdm_fft_dev.argtypes = [pi, C.c_uint32, C.c_uint32, C.c_int64, vp, C.c_uint64, C.c_uint64, vp]
        L.vit_ofdm_demod_dev.argtypes = [pi, vp, C.POINTER(OfdmShape), C.c_float, C.c_int64, vp, pr, C.c_uint64, vp]
        L.vit_ofdm_sync_dev.argtypes = [pi, C.POINTER(SyncParams), vp, C.c_int64, vp, vp, vp, vp]
        pf = C.POINTER(IqFormat)
        L.vit_ofdm_fft_iq_dev.argtypes = [pi, pf] + L.vit_ofdm_fft_dev.argtypes[1:]
        L.vit_ofdm_demod_iq_dev.argtypes = [pi, pf] + L.vit_ofdm_demod_dev.argtypes[1:]
        L.vit_ofdm_sync_iq_dev.argtypes = [pi, pf] + L.vit_ofdm_sync_dev.argtypes[1:]
        L.vit_iq_convert_dev.argtypes = [vp, pf, C.c_uint64, vp, vp]
        ps = C.POINTER(SoftRule)
        L.vit_ofdm_demap_soft_dev.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.POINTER(OfdmShape), ps, C.c_int64, vp, pr,
                                              C.c_uint64, vp, vp]
        L.vit_ofdm_demod_soft_dev.argtypes = [pi, pf, vp, C.POINTER(OfdmShape), ps, C.c_int64, vp, pr, C.c_uint64, vp, vp]
        L.vit_ofdm_acquire_dev.argtypes = [vp, C.c_uint64, pf, C.POINTER(AcqParams), C.c_int64, vp, vp, vp, vp]
        L.vit_ofdm_tii_dev.argtypes = [pi, pf, C.POINTER(TiiParams), vp, C.c_int64, vp, vp, vp]
        L.vit_tii_pair_bins.argtypes = [C.c_uint32, vp]
        L.vit_tii_pair_bins.restype = C.c_int64
        L.vit_tii_main_id.argtypes = [C.c_uint32]
        L.vit_resample_taps.argtypes = [C.c_uint32, C.c_uint32, C.c_double, vp]
        L.vit_resample_taps.restype = C.c_int64
        L.vit_resample_out_count.argtypes = [C.c_uint64, C.POINTER(ResampleParams)]
        L.vit_resample_out_count.restype = C.c_int64
        L.vit_iq_resample_dev.argtypes = [vp, C.c_uint64, pf, C.POINTER(ResampleParams), C.c_int64, vp, C.c_uint64, vp]
        L.vit_packet_fec_sync_dev.argtypes = [vp, C.c_int64, vp, vp]
        L.vit_packet_fec_count.argtypes = [C.c_int64, C.c_uint32]
        L.vit_packet_fec_count.restype = C.c_int64
        L.vit_packet_fec_dev.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp]
        L.vit_packet_fec_frame_host.argtypes = [vp, vp]
        L.vit_packets_dev.argtypes = [vp, C.c_uint32, C.c_int64, vp, vp]
        L.vit_packet_table_layout.argtypes = [vp, C.c_uint32, vp]
        L.vit_packet_table_dev.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        L.vit_data_groups_table_layout.argtypes = [vp, C.c_uint32, vp]
        L.vit_data_groups_table_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp, vp]
        L.vit_data_groups_dev.argtypes = [vp, vp, C.c_int64, vp, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.vit_data_groups_host.argtypes = [vp, vp, C.c_int64, vp, C.c_uint32, vp, vp, C.c_uint32]
        L.vit_mci_fibs_dev.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp, vp, vp]
        L.vit_mci_fibs_host.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp, vp]
        L.vit_eep_profile.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, pp, vp]
        L.vit_mci_ens_table.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        L.vit_mci_dir_dev.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp, vp, vp, vp]
        L.vit_mci_dir_host.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp, vp, vp]
        L.vit_mci_dir_ens_table.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
        L.vit_mci_pkt_table.argtypes = [vp, C.c_uint32, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp]
        _lib = L
    return _lib


def last_error():
    return lib().vit_last_error().decode()


def _check(rc, what):
    if rc != 0:
        raise ViterbiError("%s failed (rc=%d): %s" % (what, rc, last_error()))


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the reference's exports ------------------------------------------------

def initialize():
    return bool(lib().initialize())


def GetCPUCaps():
    return int(lib().GetCPUCaps())


def WakeUpYMM():
    lib().WakeUpYMM()


def device_count():
    return int(lib().vit_device_count())


def set_kernel(which):
    return int(lib().vit_set_kernel(int(which)))


def set_renorm_ge(on):
    """0: renormalise on `> 150` (reference C decoders, Rel_cpp); 1: on `>= 150` (MASM decoders, Rel_asm)"""
    return int(lib().vit_set_renorm_ge(1 if on else 0))


def set_batch_window_us(us):
    return int(lib().vit_set_batch_window_us(int(us)))


def set_batch_min_callers(n):
    return int(lib().vit_set_batch_min_callers(int(n)))


def set_batch_depth(n):
    return int(lib().vit_set_batch_depth(int(n)))


def set_batch_spin_cpus(n):
    return int(lib().vit_set_batch_spin_cpus(int(n)))


def deconvolve(framebits, symbols, unused=0, decoded=None):
    """int deconvolve(framebits, u32 symbols[4*(framebits+6)], unused, u8 out[framebits/8]).
    Returns (rc, decoded) with rc as the reference returns it (0 ok, 1 failure)."""
    symbols = np.ascontiguousarray(symbols, np.uint32)
    if symbols.size < 4 * (framebits + TAIL):
        raise ValueError("need 4*(framebits+6) symbols")
    if decoded is None:
        decoded = np.zeros((framebits + 7) // 8, np.uint8)
    rc = lib().deconvolve(framebits, _np(symbols), unused, _np(decoded))
    return int(rc), decoded


def RScheckSuperframe(p, startIx, RSDims, outVector=None):
    """int RScheckSuperframe(u8 p[120*RSDims], startIx, RSDims, u8 out[110*RSDims])."""
    p = np.ascontiguousarray(p, np.uint8)
    if p.size < 120 * RSDims:
        raise ValueError("need 120*RSDims bytes")
    if outVector is None:
        outVector = np.zeros(110 * RSDims, np.uint8)
    rc = lib().RScheckSuperframe(_np(p), startIx, RSDims, _np(outVector))
    return int(rc), outVector


# ---- batched extension, host buffers ----------------------------------------

def decode_batch_host(symbols_u8, framebits):
    symbols_u8 = np.ascontiguousarray(symbols_u8, np.uint8).reshape(-1, 4 * (framebits + TAIL))
    n = symbols_u8.shape[0]
    out = np.zeros((n, (framebits + 7) // 8), np.uint8)
    _check(lib().vit_decode_batch_host(_np(symbols_u8), _np(out), framebits, n), "vit_decode_batch_host")
    return out


def rs_batch_host(p, RSDims, out_init=None):
    p = np.ascontiguousarray(p, np.uint8).reshape(-1, 120 * RSDims)
    n = p.shape[0]
    out = (np.zeros((n, 110 * RSDims), np.uint8) if out_init is None
           else np.array(out_init, np.uint8).reshape(n, 110 * RSDims).copy())
    ret = np.zeros(n, np.int32)
    _check(lib().vit_rs_batch_host(_np(p), _np(out), _np(ret), RSDims, n), "vit_rs_batch_host")
    return ret, out


# ---- batched extension, device-resident (torch tensors are only the memory) ----

def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(int(stream))


def decode_batch_dev(d_symbols_u8, d_out, framebits, nframes, stream=None):
    """d_symbols_u8 / d_out: torch uint8 CUDA tensors (device format, see header)."""
    _check(lib().vit_decode_batch_dev(C.c_void_p(d_symbols_u8.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                      framebits, nframes, _stream_ptr(stream)), "vit_decode_batch_dev")


def decode_batch_dev_u32(d_symbols_u32, d_out, framebits, nframes, stream=None):
    _check(lib().vit_decode_batch_dev_u32(C.c_void_p(d_symbols_u32.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                          framebits, nframes, _stream_ptr(stream)), "vit_decode_batch_dev_u32")


def decode_varlen_dev(d_symbols_u8, d_out, d_desc, nframes, max_framebits, stream=None):
    _check(lib().vit_decode_varlen_dev(C.c_void_p(d_symbols_u8.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                       C.c_void_p(d_desc.data_ptr()), nframes, max_framebits,
                                       _stream_ptr(stream)), "vit_decode_varlen_dev")


def decode_varlen_dev_checked(d_symbols_u8, d_out, d_desc, nframes, max_framebits, stream=None, sym_bytes=None,
                              out_bytes=None):
    """descriptors that reach outside the two buffers (sizes default to the tensors' sizes) are skipped on the device"""
    _check(lib().vit_decode_varlen_dev_checked(
        C.c_void_p(d_symbols_u8.data_ptr()), d_symbols_u8.numel() if sym_bytes is None else sym_bytes,
        C.c_void_p(d_out.data_ptr()), d_out.numel() if out_bytes is None else out_bytes,
        C.c_void_p(d_desc.data_ptr()), nframes, max_framebits, _stream_ptr(stream)), "vit_decode_varlen_dev_checked")


def sort_descs(desc):
    """in-place, longest first (host numpy array of DESC_DTYPE)"""
    assert desc.dtype == DESC_DTYPE and desc.flags["C_CONTIGUOUS"]
    lib().vit_sort_descs(_np(desc), desc.size)
    return desc


def pack_symbols_dev(d_symbols_u32, d_symbols_u8, nsym, stream=None):
    _check(lib().vit_pack_symbols_dev(C.c_void_p(d_symbols_u32.data_ptr()), C.c_void_p(d_symbols_u8.data_ptr()),
                                      nsym, _stream_ptr(stream)), "vit_pack_symbols_dev")


def rs_batch_dev(d_p, d_out, d_ret, RSDims, nsf, stream=None):
    _check(lib().vit_rs_batch_dev(C.c_void_p(d_p.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                  C.c_void_p(d_ret.data_ptr()), RSDims, nsf, _stream_ptr(stream)),
           "vit_rs_batch_dev")


def dabplus_superframes_dev(d_symbols_u8, d_work, d_rs_out, d_ret, RSDims, nsf, stream=None):
    """decode 5*nsf frames of 192*RSDims bits, then RScheckSuperframe on every group of five"""
    _check(lib().vit_dabplus_superframes_dev(C.c_void_p(d_symbols_u8.data_ptr()), C.c_void_p(d_work.data_ptr()),
                                             C.c_void_p(d_rs_out.data_ptr()), C.c_void_p(d_ret.data_ptr()),
                                             RSDims, nsf, _stream_ptr(stream)), "vit_dabplus_superframes_dev")


def punct_profile(segments):
    """(steps, keep) pairs -> PunctProfile.  keep: an int (bit 4*(k mod 8) + j = symbol j of the segment's k-th step
    is transmitted) or a string of at most 32 '0'/'1' characters in the standard's v0...v31 order (keep = sum v_i << i).
    Validity (segment count, zero-step segments, the step sum) is the library's to judge: punctured_length()."""
    segments = list(segments)
    if len(segments) > PUNCT_MAX_SEGS:
        raise ValueError("at most %d segments" % PUNCT_MAX_SEGS)
    p = PunctProfile()
    p.nsegs = len(segments)
    for k, (steps, keep) in enumerate(segments):
        if isinstance(keep, str):
            if not keep or len(keep) > 32 or set(keep) - {"0", "1"}:
                raise ValueError("puncturing vector must be 1..32 characters '0'/'1': %r" % keep)
            keep = sum(1 << i for i, v in enumerate(keep) if v == "1")
        p.seg[k].steps = int(steps)
        p.seg[k].keep = int(keep) & 0xFFFFFFFF
    return p


def punctured_length(profile, framebits):
    """transmitted symbols of one frame under `profile`, or -1 (invalid, or steps != framebits + 6)"""
    if not isinstance(profile, PunctProfile):
        profile = punct_profile(profile)
    return int(lib().vit_punctured_length(C.byref(profile), framebits))


def decode_punctured_dev(d_punct, d_out, framebits, nframes, profile, erasure=128, stream=None):
    """d_punct: torch uint8 CUDA tensor, frame f's transmitted symbols at f*punctured_length(profile, framebits)
    (any alignment); profile: PunctProfile or (steps, keep) pairs; output as decode_batch_dev"""
    if not isinstance(profile, PunctProfile):
        profile = punct_profile(profile)
    _check(lib().vit_decode_punctured_dev(C.c_void_p(d_punct.data_ptr()), C.c_void_p(d_out.data_ptr()), framebits, nframes,
                                          C.byref(profile), int(erasure), _stream_ptr(stream)), "vit_decode_punctured_dev")


def decode_punctured_varlen_dev(d_punct, d_out, d_desc, nframes, max_framebits, d_profiles, nprofiles, erasure=128,
                                stream=None, sym_bytes=None, out_bytes=None):
    """descriptors (DESC_DTYPE on the device): sym_offset = the frame's transmitted symbols in d_punct, reserved = its
    profile's index in d_profiles (a device tensor of nprofiles PunctProfile images); checked against the buffer sizes
    (default: the tensors' sizes) like decode_varlen_dev_checked"""
    _check(lib().vit_decode_punctured_varlen_dev(
        C.c_void_p(d_punct.data_ptr()), d_punct.numel() if sym_bytes is None else sym_bytes,
        C.c_void_p(d_out.data_ptr()), d_out.numel() if out_bytes is None else out_bytes,
        C.c_void_p(d_desc.data_ptr()), nframes, max_framebits, C.c_void_p(d_profiles.data_ptr()), nprofiles, int(erasure),
        _stream_ptr(stream)), "vit_decode_punctured_varlen_dev")


def profiles_bytes(profiles):
    """host image of a profile table (PunctProfile or (steps, keep) pairs each) -> uint8 numpy array"""
    return np.frombuffer(b"".join(bytes(p if isinstance(p, PunctProfile) else punct_profile(p)) for p in profiles),
                         np.uint8).copy()


def _ptr(t):
    """device tensor -> its address, None -> NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _profile_ref(profile):
    """None (depunctured input) or a PunctProfile / (steps, keep) pairs -> the argument of the chains below"""
    if profile is None:
        return None
    return C.byref(profile if isinstance(profile, PunctProfile) else punct_profile(profile))


def prbs_bytes(framebits):
    """the energy dispersal PRBS as the XOR bytes of one frame ((framebits+7)//8, padding bits 0) -> uint8 numpy array;
    ValueError for odd framebits or framebits > 9216 (host only, needs no GPU)"""
    out = np.zeros(max((int(framebits) + 7) // 8, 1), np.uint8)
    n = lib().vit_energy_dispersal_prbs(out.ctypes.data_as(C.c_void_p), int(framebits) & 0xFFFFFFFF)
    if n < 0:
        raise ValueError("framebits must be even and <= %d: %r" % (MAX_FRAMEBITS, framebits))
    return out[:n]


def energy_dispersal_dev(d_bytes, framebits, nframes, stream=None):
    """in place: nframes frames of (framebits+7)//8 bytes back to back (torch uint8 CUDA tensor, any alignment)"""
    _check(lib().vit_energy_dispersal_dev(_ptr(d_bytes), framebits, nframes, _stream_ptr(stream)), "vit_energy_dispersal_dev")


def energy_dispersal_varlen_dev(d_bytes, d_desc, nframes, stream=None, out_bytes=None):
    """in place over the frames of a descriptor table (DESC_DTYPE on the device: out_offset, framebits); descriptors
    reaching outside out_bytes (default: d_bytes's size) or with invalid framebits are skipped"""
    _check(lib().vit_energy_dispersal_varlen_dev(_ptr(d_bytes), d_bytes.numel() if out_bytes is None else out_bytes,
                                                 _ptr(d_desc), nframes, _stream_ptr(stream)),
           "vit_energy_dispersal_varlen_dev")


def fib_crc_dev(d_fibs, nfibs, d_ok, stream=None):
    """nfibs 32-byte FIBs (descrambled) -> d_ok[i] = 1 if FIB i's CRC-16 holds, else 0"""
    _check(lib().vit_fib_crc_dev(_ptr(d_fibs), nfibs, _ptr(d_ok), _stream_ptr(stream)), "vit_fib_crc_dev")


def decode_fic_dev(d_in, d_fibs, d_fib_ok, framebits, nframes, profile=None, erasure=128, stream=None):
    """FIC chain: [depuncture ->] decode -> descramble -> FIB CRC.  profile None: d_in holds depunctured u8 symbols;
    otherwise a PunctProfile or (steps, keep) pairs and d_in the transmitted symbols.  d_fibs receives the descrambled
    frames, d_fib_ok nframes*framebits/256 flags."""
    _check(lib().vit_decode_fic_dev(_ptr(d_in), _ptr(d_fibs), _ptr(d_fib_ok), framebits, nframes, _profile_ref(profile),
                                    int(erasure), _stream_ptr(stream)), "vit_decode_fic_dev")


def dabplus_punctured_superframes_dev(d_in, profile, d_work, d_rs_out, d_ret, RSDims, nsf, d_fire_ok=None, erasure=128,
                                      stream=None):
    """DAB+ chain: [depuncture ->] decode 5*nsf frames of 192*RSDims bits into d_work -> descramble -> fire-code flag
    per superframe (d_fire_ok, optional) -> batched RScheckSuperframe into d_rs_out / d_ret.  profile as for
    decode_fic_dev."""
    _check(lib().vit_dabplus_punctured_superframes_dev(_ptr(d_in), _profile_ref(profile), int(erasure), _ptr(d_work),
                                                       _ptr(d_rs_out), _ptr(d_ret), _ptr(d_fire_ok), RSDims, nsf,
                                                       _stream_ptr(stream)), "vit_dabplus_punctured_superframes_dev")


def dabplus_aus_dev(d_sf, RSDims, nsf, d_au, d_ret=None, sf_stride=None, stream=None):
    """one AU_DTYPE record (20 bytes, in the uint8 tensor d_au) per superframe of 110*RSDims bytes at d_sf + s*sf_stride
    (default: back to back, the layout of d_rs_out); d_ret: the chain's RS return values, negative -> AU_RS_FAILED.
    sf_stride = 120*RSDims on d_work reads the superframes before RS."""
    _check(lib().vit_dabplus_aus_dev(_ptr(d_sf), 110 * RSDims if sf_stride is None else sf_stride, RSDims, nsf,
                                     _ptr(d_ret), _ptr(d_au), _stream_ptr(stream)), "vit_dabplus_aus_dev")


def dabplus_aus_host(sf, RSDims):
    """host, no GPU: the AU_DTYPE record of one superframe (110*RSDims bytes)"""
    sf = np.ascontiguousarray(sf, np.uint8).reshape(-1)
    if sf.size != 110 * RSDims:
        raise ValueError("a superframe has 110*RSDims bytes")
    out = np.zeros(1, AU_DTYPE)
    _check(lib().vit_dabplus_aus_host(_np(sf), RSDims, _np(out)), "vit_dabplus_aus_host")
    return out[0]


def fire_code_dev(d_bytes, stride, n, d_ok, stream=None):
    """d_ok[i] = the fire code of the 11 bytes at d_bytes + i*stride (stride 24*RSDims over descrambled frames: every
    logical frame as a candidate superframe start)"""
    _check(lib().vit_fire_code_dev(_ptr(d_bytes), stride, n, _ptr(d_ok), _stream_ptr(stream)), "vit_fire_code_dev")


def packet_fec_sync_dev(d_stream, nslots, d_score, stream=None):
    """d_score (103 uint32 on the device) [p] = how many slots of the stream carry the FEC packet header that phase p puts
    there; the phase of the FEC frames is the largest score's"""
    _check(lib().vit_packet_fec_sync_dev(_ptr(d_stream), nslots, _ptr(d_score), _stream_ptr(stream)), "vit_packet_fec_sync_dev")


def packet_fec_count(nslots, phase):
    """whole FEC frames in nslots slots from `phase` on"""
    n = int(lib().vit_packet_fec_count(nslots, phase))
    if n < 0:
        raise ViterbiError("vit_packet_fec_count failed: " + last_error())
    return n


def packet_fec_dev(d_stream, d_out, nslots, phase, d_fec, stream=None):
    """RS(204,188) over the packet_fec_count(nslots, phase) whole FEC frames of the stream (uint8 CUDA tensors; d_out is
    d_stream or does not overlap it); one FEC_REC_DTYPE record (16 bytes, in the uint8 tensor d_fec) per frame"""
    _check(lib().vit_packet_fec_dev(_ptr(d_stream), _ptr(d_out), nslots, phase, _ptr(d_fec), _stream_ptr(stream)),
           "vit_packet_fec_dev")


def packet_fec_frame_host(frame):
    """host, no GPU: one FEC frame of 2472 bytes -> (the decoded frame, its FEC_REC_DTYPE record)"""
    frame = np.array(frame, np.uint8).reshape(-1)
    if frame.size != FEC_FRAME_BYTES:
        raise ValueError("an FEC frame has 2472 bytes")
    out = np.zeros(1, FEC_REC_DTYPE)
    _check(lib().vit_packet_fec_frame_host(_np(frame), _np(out)), "vit_packet_fec_frame_host")
    return frame, out[0]


def packets_dev(d_bytes, framebytes, nframes, d_rec, stream=None):
    """one PACKET_REC_DTYPE record (8 bytes, in the uint8 tensor d_rec) per 24-byte slot of nframes logical frames of
    framebytes bytes"""
    _check(lib().vit_packets_dev(_ptr(d_bytes), framebytes, nframes, _ptr(d_rec), _stream_ptr(stream)), "vit_packets_dev")


def _pkt_table(tab):
    """a stream table (PKT_STREAM_DTYPE array, or anything np.asarray turns into one) -> contiguous array"""
    return np.ascontiguousarray(np.asarray(tab, PKT_STREAM_DTYPE).reshape(-1))


def packet_table_layout(tab):
    """host, no GPU: the layout of a stream table (PKT_STREAM_DTYPE) -> one PKT_LAYOUT_DTYPE record (rec_index, fec_index per
    entry; nrec, nfecrec, bytes_end); ViterbiError for a table that breaks a rule of include/viterbi_amd.h"""
    tab = _pkt_table(tab)
    out = np.zeros(1, PKT_LAYOUT_DTYPE)
    _check(lib().vit_packet_table_layout(_np(tab), tab.size, _np(out)), "vit_packet_table_layout")
    return out[0]


def packet_table_dev(d_bytes, tab, d_srec, d_fec, d_rec, d_score=None, stream=None):
    """packet mode over every stream of the table (PKT_STREAM_DTYPE) in a fixed number of launches: FEC phase found on the
    device, RS(204,188) in place in d_bytes, packet records.  uint8 CUDA tensors in the layout of packet_table_layout:
    d_srec one PKT_STREAM_REC_DTYPE record (16 bytes) per stream, d_fec FEC_REC_DTYPE records (None if nfecrec is 0), d_rec
    PACKET_REC_DTYPE records; d_score (optional) 103 uint32 per stream"""
    tab = _pkt_table(tab)
    _check(lib().vit_packet_table_dev(_ptr(d_bytes), _np(tab), tab.size, _ptr(d_srec), _ptr(d_fec), _ptr(d_rec), _ptr(d_score),
                                      _stream_ptr(stream)), "vit_packet_table_dev")


def data_groups_dev(d_bytes, d_rec, nslots, d_dg, max_groups, d_sum, d_data=None, data_capacity=0, stream=None):
    """MSC data groups of a stream of nslots slots and the records packets_dev wrote for it (uint8 CUDA tensors): up to
    max_groups DGROUP_REC_DTYPE records (32 bytes each, in d_dg), one DGROUP_SUM_DTYPE record (32 bytes, in d_sum) and,
    unless d_data is None (records only), the groups' bytes in d_data, each at its record's offset"""
    _check(lib().vit_data_groups_dev(_ptr(d_bytes), _ptr(d_rec), nslots, _ptr(d_dg), max_groups, _ptr(d_sum), _ptr(d_data),
                                     data_capacity, _stream_ptr(stream)), "vit_data_groups_dev")


def data_groups_host(stream, rec, max_groups, data_capacity):
    """host, no GPU: the same definition for a stream (bytes) and its PACKET_REC_DTYPE records -> (the written
    DGROUP_REC_DTYPE records, the DGROUP_SUM_DTYPE record, the data_capacity bytes of the groups' data with zeros between
    them); data_capacity None: records only, data is None"""
    stream = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    rec = np.ascontiguousarray(rec, PACKET_REC_DTYPE).reshape(-1)
    if stream.size != PKT_SLOT * rec.size:
        raise ValueError("one record per 24-byte slot of the stream")
    dg, summary = np.zeros(max(max_groups, 1), DGROUP_REC_DTYPE), np.zeros(1, DGROUP_SUM_DTYPE)
    data = None if data_capacity is None else np.zeros(max(data_capacity, 1), np.uint8)
    _check(lib().vit_data_groups_host(_np(stream), _np(rec), rec.size, _np(dg), max_groups, _np(summary),
                                      None if data is None else _np(data), data_capacity or 0), "vit_data_groups_host")
    return dg[:int(summary["nwritten"][0])], summary[0], None if data is None else data[:data_capacity]


def _dg_table(tab):
    """a data group table (DG_STREAM_DTYPE array, or anything np.asarray turns into one) -> contiguous array"""
    return np.ascontiguousarray(np.asarray(tab, DG_STREAM_DTYPE).reshape(-1))


def data_groups_table_layout(tab):
    """host, no GPU: the layout of a data group table (DG_STREAM_DTYPE) -> one DG_LAYOUT_DTYPE record (dg_index, data_offset
    per entry; ndg, data_bytes, bytes_end, rec_end); ViterbiError for a table that breaks a rule of include/viterbi_amd.h"""
    tab = _dg_table(tab)
    out = np.zeros(1, DG_LAYOUT_DTYPE)
    _check(lib().vit_data_groups_table_layout(_np(tab), tab.size, _np(out)), "vit_data_groups_table_layout")
    return out[0]


def data_groups_table_dev(d_bytes, d_rec, tab, d_dg, d_sum, d_data=None, stream=None):
    """data_groups_dev over every stream of the table (DG_STREAM_DTYPE) in a fixed number of launches.  uint8 CUDA tensors
    in the layout of data_groups_table_layout: d_dg DGROUP_REC_DTYPE records (stream k's from dg_index[k]), d_sum one
    DGROUP_SUM_DTYPE record (32 bytes) per stream, d_data the streams' blocks (stream k's from data_offset[k]; None: every
    stream records only); d_rec typically packet_table_dev's, with rec_index from its layout"""
    tab = _dg_table(tab)
    _check(lib().vit_data_groups_table_dev(_ptr(d_bytes), _ptr(d_rec), _np(tab), tab.size, _ptr(d_dg), _ptr(d_sum), _ptr(d_data),
                                           _stream_ptr(stream)), "vit_data_groups_table_dev")


def mci_fibs_dev(d_fibs, nfibs, G, d_sub, d_grp, d_fib_ok=None, d_status=None, stream=None):
    """FIG 0/0, 0/1 and 0/2 of nfibs 32-byte FIBs (uint8 CUDA tensors; d_fib_ok: the flags of decode_fic_dev, None = every
    FIB is used), resolved per group of G FIBs: 64 MCI_SUBCH_DTYPE records (20 bytes each, in the uint8 tensor d_sub) and
    one MCI_GROUP_DTYPE record (16 bytes, in d_grp) per group; d_status: one byte per FIB, optional"""
    _check(lib().vit_mci_fibs_dev(_ptr(d_fibs), _ptr(d_fib_ok), nfibs, G, _ptr(d_sub), _ptr(d_grp), _ptr(d_status),
                                  _stream_ptr(stream)), "vit_mci_fibs_dev")


def mci_fibs_host(fibs, G, fib_ok=None):
    """host, no GPU: the same definition -> (MCI_SUBCH_DTYPE array (ngroups, 64), MCI_GROUP_DTYPE array (ngroups,), the
    status bytes)"""
    fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G if 1 <= G <= MCI_MAX_G else 0
    sub, grp, st = np.zeros((ng, 64), MCI_SUBCH_DTYPE), np.zeros(ng, MCI_GROUP_DTYPE), np.zeros(n, np.uint8)
    ok = None if fib_ok is None else np.ascontiguousarray(fib_ok, np.uint8).reshape(n)
    _check(lib().vit_mci_fibs_host(_np(fibs), None if ok is None else _np(ok), n, G, _np(sub), _np(grp), _np(st)),
           "vit_mci_fibs_host")
    return sub, grp, st


def _keep_vectors(keep_pi):
    """24 puncturing vectors PI_1 ... PI_24 (ints, or '0'/'1' strings as for punct_profile) -> uint32 array"""
    v = [punct_profile([(8, k)]).seg[0].keep for k in keep_pi]
    if len(v) != 24:
        raise ValueError("keep_pi holds the 24 vectors PI_1 ... PI_24")
    return np.array(v, np.uint32)


def eep_profile(option, level, size_cu, keep_pi, keep_tail):
    """host, no GPU: the EEP profile of a long-form sub-channel (option 0 = A, 1 = B; level 0 ... 3) of size_cu capacity
    units from the caller's vectors -> (PunctProfile, framebits); ViterbiError where the rule has no such profile"""
    pi = _keep_vectors(keep_pi)
    tail = punct_profile([(6, keep_tail)]).seg[0].keep
    out, fb = PunctProfile(), C.c_uint32(0)
    _check(lib().vit_eep_profile(option, level, size_cu, _np(pi), tail, C.byref(out), C.byref(fb)), "vit_eep_profile")
    return out, int(fb.value)


def mci_ens_table(sub, keep_pi, keep_tail, max_profiles=64):
    """host, no GPU: one group's 64 MCI_SUBCH_DTYPE records -> (ENS_SUBCH_DTYPE rows for ensemble_dev with phase and
    nframes still 0, the list of their PunctProfile, the mask of SubChIds that are signalled but give no row)"""
    sub = np.ascontiguousarray(np.asarray(sub, MCI_SUBCH_DTYPE).reshape(-1))
    if sub.size != 64:
        raise ValueError("a group has 64 records")
    pi = _keep_vectors(keep_pi)
    tail = punct_profile([(6, keep_tail)]).seg[0].keep
    rows = np.zeros(64, ENS_SUBCH_DTYPE)
    profs = (PunctProfile * max(max_profiles, 1))()
    nsub, nprof, skipped = C.c_uint32(0), C.c_uint32(max_profiles), C.c_uint64(0)
    _check(lib().vit_mci_ens_table(_np(sub), _np(pi), tail, _np(rows), C.byref(nsub), C.byref(profs), C.byref(nprof),
                                   C.byref(skipped)), "vit_mci_ens_table")
    return rows[:nsub.value].copy(), [profs[k] for k in range(nprof.value)], int(skipped.value)


def mci_dir_dev(d_fibs, nfibs, G, d_svc, d_pkt, d_dir, d_fib_ok=None, d_status=None, stream=None):
    """the service directory of nfibs 32-byte FIBs (uint8 CUDA tensors; d_fib_ok as for mci_fibs_dev), resolved per group of
    G FIBs: 64 MCI_SERVICE_DTYPE records (32 bytes each, in d_svc), 64 MCI_PKTCOMP_DTYPE records (20 bytes each, in d_pkt)
    and one MCI_DIR_DTYPE record (40 bytes, in d_dir) per group; d_status: one byte per FIB, optional"""
    _check(lib().vit_mci_dir_dev(_ptr(d_fibs), _ptr(d_fib_ok), nfibs, G, _ptr(d_svc), _ptr(d_pkt), _ptr(d_dir), _ptr(d_status),
                                 _stream_ptr(stream)), "vit_mci_dir_dev")


def mci_dir_host(fibs, G, fib_ok=None):
    """host, no GPU: the same definition -> (MCI_SERVICE_DTYPE array (ngroups, 64), MCI_PKTCOMP_DTYPE array (ngroups, 64),
    MCI_DIR_DTYPE array (ngroups,), the status bytes)"""
    fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G if 1 <= G <= MCI_MAX_G else 0
    svc, pkt = np.zeros((ng, DIR_MAX), MCI_SERVICE_DTYPE), np.zeros((ng, DIR_MAX), MCI_PKTCOMP_DTYPE)
    d, st = np.zeros(ng, MCI_DIR_DTYPE), np.zeros(n, np.uint8)
    ok = None if fib_ok is None else np.ascontiguousarray(fib_ok, np.uint8).reshape(n)
    _check(lib().vit_mci_dir_host(_np(fibs), None if ok is None else _np(ok), n, G, _np(svc), _np(pkt), _np(d), _np(st)),
           "vit_mci_dir_host")
    return svc, pkt, d, st


def mci_dir_ens_table(sub, pkt, keep_pi, keep_tail, max_profiles=64):
    """host, no GPU: mci_ens_table with the packet-mode sub-channels that the group's MCI_PKTCOMP_DTYPE records (pkt: the
    first npkt of them, or None) name -> (rows, profiles, skipped, packet_rows: bit k marks row k as an added one)"""
    sub = np.ascontiguousarray(np.asarray(sub, MCI_SUBCH_DTYPE).reshape(-1))
    if sub.size != 64:
        raise ValueError("a group has 64 records")
    pkt = np.zeros(0, MCI_PKTCOMP_DTYPE) if pkt is None else np.ascontiguousarray(np.asarray(pkt, MCI_PKTCOMP_DTYPE).reshape(-1))
    pi = _keep_vectors(keep_pi)
    tail = punct_profile([(6, keep_tail)]).seg[0].keep
    rows = np.zeros(64, ENS_SUBCH_DTYPE)
    profs = (PunctProfile * max(max_profiles, 1))()
    nsub, nprof, skipped, marked = C.c_uint32(0), C.c_uint32(max_profiles), C.c_uint64(0), C.c_uint64(0)
    _check(lib().vit_mci_dir_ens_table(_np(sub), _np(pkt) if pkt.size else None, pkt.size, _np(pi), tail, _np(rows), C.byref(nsub),
                                       C.byref(profs), C.byref(nprof), C.byref(skipped), C.byref(marked)), "vit_mci_dir_ens_table")
    return rows[:nsub.value].copy(), [profs[k] for k in range(nprof.value)], int(skipped.value), int(marked.value)


def mci_pkt_table(rows, layout, packet_rows, fec=PKT_FEC_NONE, min_score=0):
    """host, no GPU: the rows of mci_dir_ens_table (nframes filled), their ensemble_layout record and the mask of packet rows
    -> (PKT_STREAM_DTYPE table for packet_table_dev, one stream per marked row; the row of every stream)"""
    rows = _ens_table(rows)
    lay = np.ascontiguousarray(np.asarray(layout, ENS_LAYOUT_DTYPE).reshape(1))
    tab, row_of = np.zeros(PKT_MAX_STREAMS, PKT_STREAM_DTYPE), np.zeros(PKT_MAX_STREAMS, np.uint32)
    n = C.c_uint32(0)
    _check(lib().vit_mci_pkt_table(_np(rows), rows.size, _np(lay), packet_rows, fec, min_score, _np(tab), C.byref(n), _np(row_of)),
           "vit_mci_pkt_table")
    return tab[:n.value].copy(), row_of[:n.value].copy()


def cif_ring(d_ring, first_row):
    """a C-contiguous 2-D uint8 CUDA tensor (nrows, row_bytes) of CIF rows + the row of the call's frame 0 -> CifRing"""
    if d_ring.dim() != 2 or str(d_ring.dtype) != "torch.uint8" or not d_ring.is_contiguous() or not d_ring.is_cuda:
        raise ValueError("the ring must be a C-contiguous 2-D uint8 CUDA tensor (nrows, row_bytes)")
    r = CifRing()
    r.d_base = d_ring.data_ptr()
    r.row_bytes = d_ring.shape[1]
    r.nrows = d_ring.shape[0]
    r.first_row = int(first_row)
    return r


def time_deinterleave_dev(d_ring, first_row, col, ncols, d_out, nframes, stream=None):
    """MSC time de-interleaving (include/viterbi_amd.h): frame n's ncols bytes, byte i from ring row
    (first_row + n + F[i % 16]) % nrows, column col + i, to d_out[n*ncols:(n+1)*ncols]"""
    _check(lib().vit_time_deinterleave_dev(C.byref(cif_ring(d_ring, first_row)), col, ncols, _ptr(d_out), nframes,
                                           _stream_ptr(stream)), "vit_time_deinterleave_dev")


def decode_punctured_ti_dev(d_ring, first_row, col, d_out, framebits, nframes, profile, erasure=128, stream=None):
    """one sub-channel at columns [col, col + punctured_length(profile, framebits)) of the ring, decoded over nframes
    logical frames (de-interleave fused into the depuncturing); output as decode_punctured_dev"""
    if not isinstance(profile, PunctProfile):
        profile = punct_profile(profile)
    _check(lib().vit_decode_punctured_ti_dev(C.byref(cif_ring(d_ring, first_row)), col, _ptr(d_out), framebits, nframes,
                                             C.byref(profile), int(erasure), _stream_ptr(stream)),
           "vit_decode_punctured_ti_dev")


def dabplus_ti_superframes_dev(d_ring, first_row, col, profile, d_work, d_rs_out, d_ret, RSDims, nsf, d_fire_ok=None,
                               erasure=128, stream=None):
    """the DAB+ chain of dabplus_punctured_superframes_dev from the ring: 5*nsf logical frames (5*nsf + 15 rows);
    profile required"""
    if not isinstance(profile, PunctProfile):
        profile = punct_profile(profile)
    _check(lib().vit_dabplus_ti_superframes_dev(C.byref(cif_ring(d_ring, first_row)), col, C.byref(profile), int(erasure),
                                                _ptr(d_work), _ptr(d_rs_out), _ptr(d_ret), _ptr(d_fire_ok), RSDims, nsf,
                                                _stream_ptr(stream)), "vit_dabplus_ti_superframes_dev")


def _ens_table(sub):
    """a sub-channel table (ENS_SUBCH_DTYPE array, or anything np.asarray turns into one) -> contiguous array"""
    return np.ascontiguousarray(np.asarray(sub, ENS_SUBCH_DTYPE).reshape(-1))


def ensemble_layout(sub):
    """host, no GPU: the layout of a sub-channel table (ENS_SUBCH_DTYPE) -> one ENS_LAYOUT_DTYPE record (work_offset,
    rs_offset, rec_index per entry; work_bytes, rs_bytes, nrec, rows_needed, max_framebits); ViterbiError for a table that
    breaks a rule of include/viterbi_amd.h"""
    sub = _ens_table(sub)
    out = np.zeros(1, ENS_LAYOUT_DTYPE)
    _check(lib().vit_ensemble_layout(_np(sub), sub.size, _np(out)), "vit_ensemble_layout")
    return out[0]


def rs_table_dev(d_work, d_rs_out, d_ret, sub, stream=None):
    """batched RScheckSuperframe over every DAB+ sub-channel of the table in one launch: d_work / d_rs_out in the layout
    of ensemble_layout, d_ret (int32) one value per record"""
    sub = _ens_table(sub)
    _check(lib().vit_rs_table_dev(_ptr(d_work), _ptr(d_rs_out), _ptr(d_ret), _np(sub), sub.size, _stream_ptr(stream)),
           "vit_rs_table_dev")


def dabplus_aus_table_dev(d_sf, sub, d_au, d_ret=None, from_work=False, stream=None):
    """one AU_DTYPE record per superframe of every DAB+ sub-channel of the table in one launch; d_sf in the layout of
    d_rs_out, or with from_work of d_work (the superframes before RS: the salvage pass, with d_ret None)"""
    sub = _ens_table(sub)
    _check(lib().vit_dabplus_aus_table_dev(_ptr(d_sf), 1 if from_work else 0, _np(sub), sub.size, _ptr(d_ret), _ptr(d_au),
                                           _stream_ptr(stream)), "vit_dabplus_aus_table_dev")


def ensemble_dev(d_ring, first_row, msc_col, sub, d_profiles, nprofiles, d_work, d_rs_out, d_ret, d_fire_ok=None, d_au=None,
                 erasure=128, stream=None):
    """every sub-channel of the table from the ring in one chain: de-interleave, depuncture (d_profiles: the device
    image of profiles_bytes), decode, descramble, fire code, RS, access units; outputs in the layout of ensemble_layout"""
    sub = _ens_table(sub)
    _check(lib().vit_ensemble_dev(C.byref(cif_ring(d_ring, first_row)), msc_col, _np(sub), sub.size, _ptr(d_profiles),
                                  nprofiles, int(erasure), _ptr(d_work), _ptr(d_rs_out), _ptr(d_ret), _ptr(d_fire_ok),
                                  _ptr(d_au), _stream_ptr(stream)), "vit_ensemble_dev")


def freq_interleave_bins(nfft):
    """the standard's frequency interleaving as FFT bins (include/viterbi_amd.h): QPSK symbol n of an OFDM symbol travels
    in bin result[n]; 3*nfft/4 entries -> uint16 numpy array; ValueError for nfft not in 256, 512, 1024, 2048 (host only,
    needs no GPU)"""
    out = np.zeros(8192, np.uint16)
    n = lib().vit_freq_interleave_bins(int(nfft) & 0xFFFFFFFF, _np(out))
    if n < 0:
        raise ValueError("nfft must be 256, 512, 1024 or 2048: %r" % (nfft,))
    return out[:n].copy()


def ofdm_demap_dev(d_fft, shape, d_bins, gain, nframes, d_fic=None, d_ring=None, first_row=0, col=0, sym_stride=None,
                   frame_stride=None, stream=None):
    """From the FFT (include/viterbi_amd.h): d_fft a complex64 or (re, im)-interleaved float32 CUDA tensor of nframes
    frames; shape an OfdmShape or its 5 numbers; d_bins a uint16 CUDA tensor of K FFT bins (torch has no uint16
    arithmetic: build it with freq_interleave_bins and torch.from_numpy(bins.view(np.int16)).cuda(), any 2-byte dtype
    is taken); d_fic receives the FIC symbols' soft bytes and the rows of d_ring (as cif_ring) the CIFs, either may be
    None.  Strides count complex elements and default to nfft and nsyms*sym_stride."""
    if not isinstance(shape, OfdmShape):
        shape = OfdmShape(*[int(v) for v in shape])
    if not d_fft.is_cuda or str(d_fft.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_fft must be a complex64 or float32 CUDA tensor")
    if not d_bins.is_cuda or d_bins.element_size() != 2:
        raise ValueError("d_bins must be a CUDA tensor of 2-byte elements (uint16 bins)")
    if sym_stride is None:
        sym_stride = shape.nfft
    if frame_stride is None:
        frame_stride = shape.nsyms * sym_stride
    ring = None if d_ring is None else C.byref(cif_ring(d_ring, first_row))
    _check(lib().vit_ofdm_demap_dev(_ptr(d_fft), sym_stride, frame_stride, _ptr(d_bins), C.byref(shape), float(gain), nframes,
                                    _ptr(d_fic), ring, col, _stream_ptr(stream)), "vit_ofdm_demap_dev")


def fft_twiddles(nfft):
    """the FFT's twiddles (include/viterbi_amd.h, "From the samples"): nfft/2 pairs (cos, -sin)(2 pi k / nfft) -> float32
    numpy array (nfft/2, 2); ValueError unless nfft is a power of two 64 ... 8192 (host only, needs no GPU)"""
    out = np.zeros((4096, 2), np.float32)
    n = lib().vit_fft_twiddles(int(nfft) & 0xFFFFFFFF, _np(out))
    if n < 0:
        raise ValueError("nfft must be a power of two 64 ... 8192: %r" % (nfft,))
    return out[:n].copy()


def nco_table(bits):
    """the phasors of the fine-frequency rotation: 2^bits pairs (cos, +sin)(2 pi k / 2^bits) -> float32 numpy array
    (2^bits, 2); ValueError unless 1 <= bits <= 20 (host only, needs no GPU)"""
    if not 1 <= int(bits) <= 20:
        raise ValueError("bits must be 1 ... 20: %r" % (bits,))
    out = np.zeros((1 << int(bits), 2), np.float32)
    n = lib().vit_nco_table(int(bits), _np(out))
    if n != out.shape[0]:
        raise ValueError("bits must be 1 ... 20: %r" % (bits,))
    return out


def _iq_samples(d_iq, iq_format):
    """complex samples a CUDA tensor of the format holds; ValueError for a tensor of another type"""
    if iq_format == IQ_F32:
        if not d_iq.is_cuda or str(d_iq.dtype) not in ("torch.complex64", "torch.float32"):
            raise ValueError("d_iq must be a complex64 or float32 CUDA tensor")
        return d_iq.numel() if str(d_iq.dtype) == "torch.complex64" else d_iq.numel() // 2
    if iq_format not in _IQ_DTYPES:
        raise ValueError("iq_format must be one of IQ_F32, IQ_CU8, IQ_CS8, IQ_CS16: %r" % (iq_format,))
    if not d_iq.is_cuda or str(d_iq.dtype) != _IQ_DTYPES[iq_format]:
        raise ValueError("d_iq must be a %s CUDA tensor of (I, Q) pairs for this iq_format" % _IQ_DTYPES[iq_format][6:])
    return d_iq.numel() // 2


def iq_input(d_iq, d_tw, sym_stride, frame_stride=0, d_start=None, d_nco=None, nco_bits=0, d_rot=None, nsamples=None,
             iq_format=IQ_F32, iq_scale=1.0):
    """device tensors -> IqInput.  d_iq: complex64 or (re, im)-interleaved float32 CUDA tensor - with iq_format IQ_CU8,
    IQ_CS8 or IQ_CS16 a uint8, int8 or int16 CUDA tensor of (I, Q) pairs, for the *_iq_dev calls; d_tw / d_nco: float32
    CUDA tensors from fft_twiddles / nco_table; d_start: int64 CUDA tensor of frame starts; d_rot: CUDA tensor of 4-byte
    elements, {phase0, step} per frame (torch has no uint32 arithmetic: upload a numpy uint32 array viewed as int32).
    nsamples defaults to all of d_iq, counted in complex samples of its format.  iq_scale is not stored here: it travels
    in the IqFormat of the call."""
    total = _iq_samples(d_iq, iq_format)
    if not d_tw.is_cuda or str(d_tw.dtype) != "torch.float32" or (d_nco is not None and str(d_nco.dtype) != "torch.float32"):
        raise ValueError("d_tw and d_nco must be float32 CUDA tensors")
    if d_start is not None and (not d_start.is_cuda or str(d_start.dtype) != "torch.int64"):
        raise ValueError("d_start must be an int64 CUDA tensor")
    if d_rot is not None and (not d_rot.is_cuda or d_rot.element_size() != 4):
        raise ValueError("d_rot must be a CUDA tensor of 4-byte elements (uint32 pairs)")
    a = IqInput()
    a.d_iq = d_iq.data_ptr()
    a.nsamples = total if nsamples is None else int(nsamples)
    a.sym_stride = int(sym_stride)
    a.frame_stride = int(frame_stride or 0)
    a.d_start = None if d_start is None else d_start.data_ptr()
    a.d_tw = d_tw.data_ptr()
    a.d_nco = None if d_nco is None else d_nco.data_ptr()
    a.nco_bits = int(nco_bits)
    a.d_rot = None if d_rot is None else d_rot.data_ptr()
    return a


def iq_convert_dev(d_iq, iq_format, iq_scale, d_out, nsamples=None, stream=None):
    """Integer sample formats (include/viterbi_amd.h): the floats the front end makes of the samples, written to d_out
    (complex64 or float32 CUDA tensor).  d_iq: uint8, int8 or int16 CUDA tensor of (I, Q) pairs as iq_format says;
    nsamples defaults to all of d_iq."""
    total = _iq_samples(d_iq, iq_format)
    if not d_out.is_cuda or str(d_out.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_out must be a complex64 or float32 CUDA tensor")
    n = total if nsamples is None else int(nsamples)
    if d_out.numel() * d_out.element_size() < 8 * n or n > total:
        raise ValueError("d_iq and d_out must hold nsamples complex samples")
    fmt = IqFormat(int(iq_format), float(iq_scale))
    _check(lib().vit_iq_convert_dev(_ptr(d_iq), C.byref(fmt), n, _ptr(d_out), _stream_ptr(stream)), "vit_iq_convert_dev")


def ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_tw, sym_stride, d_fft, frame_stride=None, d_start=None, d_nco=None,
                 nco_bits=0, d_rot=None, out_sym_stride=None, out_frame_stride=None, stream=None, nsamples=None,
                 iq_format=IQ_F32, iq_scale=1.0):
    """From the samples (include/viterbi_amd.h): rotation and FFT of symbols 0 ... nsyms-1 of nframes frames into d_fft
    (complex64 or float32 CUDA tensor) in the layout ofdm_demap_dev reads.  Input arguments as iq_input; frame_stride is
    required unless d_start is given; the output strides count complex elements and default to nfft and
    nsyms*out_sym_stride.  With an integer iq_format (and its iq_scale) d_iq holds the receiver's own samples."""
    if not d_fft.is_cuda or str(d_fft.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_fft must be a complex64 or float32 CUDA tensor")
    if frame_stride is None and d_start is None:
        raise ValueError("frame_stride or d_start is required")
    inp = iq_input(d_iq, d_tw, sym_stride, frame_stride, d_start, d_nco, nco_bits, d_rot, nsamples, iq_format)
    if out_sym_stride is None:
        out_sym_stride = int(nfft)
    if out_frame_stride is None:
        out_frame_stride = int(nsyms) * out_sym_stride
    if iq_format != IQ_F32:
        fmt = IqFormat(int(iq_format), float(iq_scale))
        _check(lib().vit_ofdm_fft_iq_dev(C.byref(inp), C.byref(fmt), int(nfft), int(nsyms), nframes, _ptr(d_fft), out_sym_stride,
                                         out_frame_stride, _stream_ptr(stream)), "vit_ofdm_fft_iq_dev")
        return
    _check(lib().vit_ofdm_fft_dev(C.byref(inp), int(nfft), int(nsyms), nframes, _ptr(d_fft), out_sym_stride, out_frame_stride,
                                  _stream_ptr(stream)), "vit_ofdm_fft_dev")


def ofdm_demod_dev(d_iq, shape, d_bins, gain, nframes, d_tw, sym_stride, frame_stride=None, d_start=None, d_nco=None,
                   nco_bits=0, d_rot=None, d_fic=None, d_ring=None, first_row=0, col=0, stream=None, nsamples=None,
                   iq_format=IQ_F32, iq_scale=1.0):
    """From the samples (include/viterbi_amd.h): rotation, FFT and the demapping of ofdm_demap_dev in one kernel, no spectrum
    in memory.  Input arguments as iq_input (frame_stride is required unless d_start is given); shape, d_bins, gain,
    d_fic, d_ring, first_row and col as ofdm_demap_dev.  With an integer iq_format (and its iq_scale) d_iq holds the
    receiver's own samples."""
    if not isinstance(shape, OfdmShape):
        shape = OfdmShape(*[int(v) for v in shape])
    if not d_bins.is_cuda or d_bins.element_size() != 2:
        raise ValueError("d_bins must be a CUDA tensor of 2-byte elements (uint16 bins)")
    if frame_stride is None and d_start is None:
        raise ValueError("frame_stride or d_start is required")
    inp = iq_input(d_iq, d_tw, sym_stride, frame_stride, d_start, d_nco, nco_bits, d_rot, nsamples, iq_format)
    ring = None if d_ring is None else C.byref(cif_ring(d_ring, first_row))
    if iq_format != IQ_F32:
        fmt = IqFormat(int(iq_format), float(iq_scale))
        _check(lib().vit_ofdm_demod_iq_dev(C.byref(inp), C.byref(fmt), _ptr(d_bins), C.byref(shape), float(gain), nframes,
                                           _ptr(d_fic), ring, col, _stream_ptr(stream)), "vit_ofdm_demod_iq_dev")
        return
    _check(lib().vit_ofdm_demod_dev(C.byref(inp), _ptr(d_bins), C.byref(shape), float(gain), nframes, _ptr(d_fic), ring, col,
                                    _stream_ptr(stream)), "vit_ofdm_demod_dev")


def _soft_rule(rule, gain, d_level, shape, nframes):
    """SoftRule of the *_soft_dev wrappers; ValueError for a rule that is none of the two or a d_level that cannot hold
    nframes * (nsyms - 1) floats"""
    if rule not in (SOFT_PER_CARRIER, SOFT_PER_SYMBOL):
        raise ValueError("rule must be SOFT_PER_CARRIER or SOFT_PER_SYMBOL: %r" % (rule,))
    if d_level is not None and (not d_level.is_cuda or str(d_level.dtype) != "torch.float32"
                                or d_level.numel() < nframes * (shape.nsyms - 1)):
        raise ValueError("d_level must be a float32 CUDA tensor of nframes * (nsyms - 1) elements")
    return SoftRule(int(rule), float(gain))


def ofdm_demap_soft_dev(d_fft, shape, d_bins, rule, gain, nframes, d_fic=None, d_ring=None, first_row=0, col=0,
                        d_level=None, sym_stride=None, frame_stride=None, stream=None):
    """Channel-state weighting (include/viterbi_amd.h): ofdm_demap_dev with a soft-decision rule in the place of its gain.
    rule SOFT_PER_SYMBOL scales a symbol's carriers by the symbol's mean level (gain 64 ... 128 suits the decoders);
    SOFT_PER_CARRIER is ofdm_demap_dev itself.  d_level: optional float32 CUDA tensor of nframes * (nsyms - 1) elements
    that receives every demapped symbol's level (SOFT_PER_SYMBOL only)."""
    if not isinstance(shape, OfdmShape):
        shape = OfdmShape(*[int(v) for v in shape])
    soft = _soft_rule(rule, gain, d_level, shape, nframes)
    if not d_fft.is_cuda or str(d_fft.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_fft must be a complex64 or float32 CUDA tensor")
    if not d_bins.is_cuda or d_bins.element_size() != 2:
        raise ValueError("d_bins must be a CUDA tensor of 2-byte elements (uint16 bins)")
    if sym_stride is None:
        sym_stride = shape.nfft
    if frame_stride is None:
        frame_stride = shape.nsyms * sym_stride
    ring = None if d_ring is None else C.byref(cif_ring(d_ring, first_row))
    _check(lib().vit_ofdm_demap_soft_dev(_ptr(d_fft), sym_stride, frame_stride, _ptr(d_bins), C.byref(shape), C.byref(soft),
                                         nframes, _ptr(d_fic), ring, col, _ptr(d_level), _stream_ptr(stream)),
           "vit_ofdm_demap_soft_dev")


def ofdm_demod_soft_dev(d_iq, shape, d_bins, rule, gain, nframes, d_tw, sym_stride, frame_stride=None, d_start=None,
                        d_nco=None, nco_bits=0, d_rot=None, d_fic=None, d_ring=None, first_row=0, col=0, d_level=None,
                        stream=None, nsamples=None, iq_format=IQ_F32, iq_scale=1.0):
    """Channel-state weighting (include/viterbi_amd.h): ofdm_demod_dev with a soft-decision rule in the place of its gain;
    rule, gain and d_level as ofdm_demap_soft_dev, every other argument as ofdm_demod_dev (integer sample formats
    included)."""
    if not isinstance(shape, OfdmShape):
        shape = OfdmShape(*[int(v) for v in shape])
    soft = _soft_rule(rule, gain, d_level, shape, nframes)
    if not d_bins.is_cuda or d_bins.element_size() != 2:
        raise ValueError("d_bins must be a CUDA tensor of 2-byte elements (uint16 bins)")
    if frame_stride is None and d_start is None:
        raise ValueError("frame_stride or d_start is required")
    inp = iq_input(d_iq, d_tw, sym_stride, frame_stride, d_start, d_nco, nco_bits, d_rot, nsamples, iq_format)
    ring = None if d_ring is None else C.byref(cif_ring(d_ring, first_row))
    fmt = None if iq_format == IQ_F32 else C.byref(IqFormat(int(iq_format), float(iq_scale)))
    _check(lib().vit_ofdm_demod_soft_dev(C.byref(inp), fmt, _ptr(d_bins), C.byref(shape), C.byref(soft), nframes, _ptr(d_fic),
                                         ring, col, _ptr(d_level), _stream_ptr(stream)), "vit_ofdm_demod_soft_dev")


def ofdm_sync_dev(d_iq, nfft, nsyms, nframes, d_tw, sym_stride, d_nco, nco_bits, d_prs, d_start_out, d_rot_out, W, M,
                  cp_symbols=None, thr=0.5, backoff=0, frame_stride=None, first_start=0, d_start=None, d_info=None,
                  stream=None, nsamples=None, iq_format=IQ_F32, iq_scale=1.0):
    """From the coarse start (include/viterbi_amd.h): per frame the fine start and the carrier offset, written as the
    tables ofdm_demod_dev reads - d_start_out (int64 CUDA tensor, nframes) and d_rot_out (CUDA tensor of 4-byte elements,
    {0, step} per frame).  Input arguments as iq_input; the coarse starts are d_start (d_start_out may be the same
    tensor) or first_start + t*frame_stride.  d_prs: the transmitted phase reference symbol, nfft values in FFT order
    (complex64 or float32 CUDA tensor); cp_symbols defaults to nsyms - 1; d_info (optional): CUDA tensor of 4-byte
    elements, 8 words per frame.  With an integer iq_format (and its iq_scale) d_iq holds the receiver's own samples."""
    if d_nco is None:
        raise ValueError("d_nco is required")
    if frame_stride is None and d_start is None:
        raise ValueError("frame_stride or d_start is required")
    if not d_prs.is_cuda or str(d_prs.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_prs must be a complex64 or float32 CUDA tensor")
    if d_prs.numel() * d_prs.element_size() < 8 * int(nfft):
        raise ValueError("d_prs must hold nfft complex values")
    if not d_start_out.is_cuda or str(d_start_out.dtype) != "torch.int64" or d_start_out.numel() < nframes:
        raise ValueError("d_start_out must be an int64 CUDA tensor of nframes elements")
    if not d_rot_out.is_cuda or d_rot_out.element_size() != 4 or d_rot_out.numel() < 2 * nframes:
        raise ValueError("d_rot_out must be a CUDA tensor of 2*nframes 4-byte elements (uint32 pairs)")
    if d_info is not None and (not d_info.is_cuda or d_info.element_size() != 4 or d_info.numel() < 8 * nframes):
        raise ValueError("d_info must be a CUDA tensor of 8*nframes 4-byte elements")
    inp = iq_input(d_iq, d_tw, sym_stride, frame_stride, d_start, d_nco, nco_bits, None, nsamples, iq_format)
    par = SyncParams(int(nfft), int(nsyms), int(nsyms) - 1 if cp_symbols is None else int(cp_symbols), int(W), int(M),
                     float(thr), int(backoff), int(first_start))
    if iq_format != IQ_F32:
        fmt = IqFormat(int(iq_format), float(iq_scale))
        _check(lib().vit_ofdm_sync_iq_dev(C.byref(inp), C.byref(fmt), C.byref(par), _ptr(d_prs), nframes, _ptr(d_start_out),
                                          _ptr(d_rot_out), _ptr(d_info), _stream_ptr(stream)), "vit_ofdm_sync_iq_dev")
        return
    _check(lib().vit_ofdm_sync_dev(C.byref(inp), C.byref(par), _ptr(d_prs), nframes, _ptr(d_start_out), _ptr(d_rot_out),
                                   _ptr(d_info), _stream_ptr(stream)), "vit_ofdm_sync_dev")


def ofdm_acquire_dev(d_iq, B, null_blocks, ref_blocks, period_blocks, thr, nperiods, d_start_out, first=0, offset=0,
                     d_info=None, d_power=None, nsamples=None, stream=None, iq_format=IQ_F32, iq_scale=1.0):
    """From the stream (include/viterbi_amd.h): the null-symbol search.  d_iq as iq_input (nsamples defaults to all of
    it); per frame period of period_blocks blocks of B samples one coarse start into d_start_out (int64 CUDA tensor,
    nperiods), the table ofdm_sync_dev takes as d_start; -1 where no edge passed thr.  d_info (optional): CUDA tensor of
    4-byte elements, 4 words per period; d_power (optional): float32 CUDA tensor of (nsamples - first) // B block powers."""
    total = _iq_samples(d_iq, iq_format)
    n = total if nsamples is None else int(nsamples)
    if n > total:
        raise ValueError("d_iq must hold nsamples complex samples")
    if not d_start_out.is_cuda or str(d_start_out.dtype) != "torch.int64" or d_start_out.numel() < nperiods:
        raise ValueError("d_start_out must be an int64 CUDA tensor of nperiods elements")
    if d_info is not None and (not d_info.is_cuda or d_info.element_size() != 4 or d_info.numel() < 4 * nperiods):
        raise ValueError("d_info must be a CUDA tensor of 4*nperiods 4-byte elements")
    nblk = max(n - int(first), 0) // int(B) if B else 0
    if d_power is not None and (not d_power.is_cuda or str(d_power.dtype) != "torch.float32" or d_power.numel() < nblk):
        raise ValueError("d_power must be a float32 CUDA tensor of (nsamples - first) // B elements")
    par = AcqParams(int(B), int(null_blocks), int(ref_blocks), int(period_blocks), float(thr), 0, int(first), int(offset))
    fmt = None if iq_format == IQ_F32 else C.byref(IqFormat(int(iq_format), float(iq_scale)))
    _check(lib().vit_ofdm_acquire_dev(_ptr(d_iq), n, fmt, C.byref(par), nperiods, _ptr(d_start_out), _ptr(d_info),
                                      _ptr(d_power), _stream_ptr(stream)), "vit_ofdm_acquire_dev")


def resample_taps(L, T, cutoff):
    """Before the stream (include/viterbi_amd.h): the Blackman-windowed sinc of vit_resample_taps, cutoff in cycles per
    input sample -> float32 numpy array (L, T), row phi the taps of phase phi; ValueError for an argument out of range
    (host only, needs no GPU)"""
    if not (1 <= int(L) <= 1024 and 4 <= int(T) <= 128):
        raise ValueError("L must be 1 ... 1024 and T a multiple of 4, 4 ... 128: %r, %r" % (L, T))
    out = np.zeros((int(L), int(T)), np.float32)
    if lib().vit_resample_taps(int(L), int(T), float(cutoff), _np(out)) != out.size:
        raise ValueError("L*T must be <= 16384, T a multiple of 4 and 0 < cutoff <= 0.5: %r, %r, %r" % (L, T, cutoff))
    return out


def resample_out_count(nsamples, L, M, T, pos0=0):
    """the most outputs vit_iq_resample_dev forms from nsamples samples (host only, needs no GPU); ValueError for L, M or
    T out of range"""
    for v in (nsamples, L, M, T, pos0):
        if int(v) < 0:
            raise ValueError("nsamples, L, M, T and pos0 must not be negative")
    par = ResampleParams(int(L) & 0xFFFFFFFF, int(M) & 0xFFFFFFFF, int(T) & 0xFFFFFFFF, 1, int(pos0), None, None, 0, 0, None)
    n = lib().vit_resample_out_count(int(nsamples), C.byref(par))
    if n < 0:
        raise ValueError("L must be 1 ... 1024, M 1 ... 4096, T a multiple of 4, 4 ... 128, L*T <= 16384: %r, %r, %r" % (L, M, T))
    return n


def resample_tile(L, M, T):
    """-> (outputs one workgroup of vit_iq_resample_dev forms, whether its threads read their samples from memory): the
    rule of csrc/vit_resample.hip (resample_tile there), restated for the tests that place nout around a tile's edge"""
    if M > L * T:
        return 512, True
    tile = 1024
    while tile > 1 and ((tile - 1) * M + L - 1) // L + T > 2048:
        tile //= 2
    return tile, False


def iq_resample_dev(d_iq, L, M, d_taps, nout, d_out, pos0=0, rot=None, d_nco=None, nco_bits=0, out_stride=None, nsamples=None,
                    stream=None, iq_format=IQ_F32, iq_scale=1.0):
    """Before the stream (include/viterbi_amd.h): frequency shift, low-pass and rate change by L/M.  d_iq as iq_input
    (nsamples defaults to all of it); d_taps: float32 CUDA tensor (L, T) from resample_taps; rot: None, or nchan pairs
    (phase0, step) - a sequence or a numpy array, read during the call - with d_nco, a float32 CUDA tensor from nco_table,
    and its nco_bits; d_out: complex64 or float32 CUDA tensor, channel c's nout outputs from complex element c*out_stride
    on (out_stride defaults to nout)."""
    total = _iq_samples(d_iq, iq_format)
    n = total if nsamples is None else int(nsamples)
    if n > total:
        raise ValueError("d_iq must hold nsamples complex samples")
    if not d_taps.is_cuda or str(d_taps.dtype) != "torch.float32" or d_taps.dim() != 2 or d_taps.shape[0] != int(L) or \
            not d_taps.is_contiguous():
        raise ValueError("d_taps must be a contiguous float32 CUDA tensor (L, T)")
    if d_nco is not None and (not d_nco.is_cuda or str(d_nco.dtype) != "torch.float32"):
        raise ValueError("d_nco must be a float32 CUDA tensor")
    if not d_out.is_cuda or str(d_out.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("d_out must be a complex64 or float32 CUDA tensor")
    pairs = None if rot is None else np.ascontiguousarray(np.asarray(rot, np.int64).reshape(-1, 2) & 0xFFFFFFFF, np.uint32)
    nchan = 1 if pairs is None else pairs.shape[0]
    stride = int(nout) if out_stride is None else int(out_stride)
    if nout < 0 or stride < 0 or d_out.numel() * d_out.element_size() < 8 * ((nchan - 1) * stride + nout):
        raise ValueError("d_out must hold nchan channels of nout complex samples at out_stride")
    par = ResampleParams(int(L), int(M), int(d_taps.shape[1]), nchan, int(pos0), d_taps.data_ptr(),
                         None if d_nco is None else d_nco.data_ptr(), int(nco_bits), 0,
                         None if pairs is None else pairs.ctypes.data)
    fmt = None if iq_format == IQ_F32 else C.byref(IqFormat(int(iq_format), float(iq_scale)))
    _check(lib().vit_iq_resample_dev(_ptr(d_iq), n, fmt, C.byref(par), int(nout), _ptr(d_out), stride, _stream_ptr(stream)),
           "vit_iq_resample_dev")


def ofdm_tii_dev(d_iq, nfft, nframes, d_tw, d_pairs, d_tii, ngroups=8, ncombs=24, nrep=4, navg=8, thr=2.5, offset=0,
                 d_start=None, frame_stride=None, d_nco=None, nco_bits=0, d_rot=None, d_energy=None, nsamples=None, stream=None,
                 iq_format=IQ_F32, iq_scale=1.0):
    """Transmitter identification (include/viterbi_amd.h): per frame the window of nfft samples at the frame's start +
    offset - the null symbol; mode I behind ofdm_sync_dev: offset = -sym_stride -, per group of navg frames 2 + 2*ncombs
    words into d_tii (CUDA tensor of 4-byte elements): {nused, noise, mask[0], strength[0], ...}, which tii_records views.
    Input arguments as iq_input (d_start, or frame_stride, is required; d_rot is the table ofdm_sync_dev wrote); d_pairs:
    CUDA tensor of 2-byte elements, nrep*ngroups*ncombs lower bins (tii_pair_bins(1) for mode I); d_energy (optional):
    float32 CUDA tensor of ngrp*ngroups*ncombs group energies."""
    if frame_stride is None and d_start is None:
        raise ValueError("frame_stride or d_start is required")
    slots = int(ngroups) * int(ncombs)
    ngrp = -(-int(nframes) // int(navg)) if navg and nframes > 0 else 0
    if not d_pairs.is_cuda or d_pairs.element_size() != 2 or d_pairs.numel() < int(nrep) * slots:
        raise ValueError("d_pairs must be a CUDA tensor of nrep*ngroups*ncombs 2-byte elements (uint16 bins)")
    if not d_tii.is_cuda or d_tii.element_size() != 4 or d_tii.numel() < ngrp * (2 + 2 * int(ncombs)):
        raise ValueError("d_tii must be a CUDA tensor of ceil(nframes/navg) * (2 + 2*ncombs) 4-byte elements")
    if d_energy is not None and (not d_energy.is_cuda or str(d_energy.dtype) != "torch.float32" or d_energy.numel() < ngrp * slots):
        raise ValueError("d_energy must be a float32 CUDA tensor of ceil(nframes/navg) * ngroups*ncombs elements")
    inp = iq_input(d_iq, d_tw, 0, frame_stride, d_start, d_nco, nco_bits, d_rot, nsamples, iq_format)
    if inp.nsamples > _iq_samples(d_iq, iq_format):
        raise ValueError("d_iq must hold nsamples complex samples")
    par = TiiParams(int(nfft), int(ngroups), int(ncombs), int(nrep), int(navg), float(thr), int(offset))
    fmt = None if iq_format == IQ_F32 else C.byref(IqFormat(int(iq_format), float(iq_scale)))
    _check(lib().vit_ofdm_tii_dev(C.byref(inp), fmt, C.byref(par), _ptr(d_pairs), nframes, _ptr(d_tii), _ptr(d_energy),
                                  _stream_ptr(stream)), "vit_ofdm_tii_dev")


def tii_pair_bins(mode):
    """the standard's TII carrier pairs as the d_pairs table of ofdm_tii_dev: uint16 numpy array (R, Gp, C) of lower FFT
    bins - mode 1: (4, 8, 24) at nfft 2048; ValueError for any other mode (host only, needs no GPU)"""
    out = np.zeros(768, np.uint16)
    n = lib().vit_tii_pair_bins(int(mode) & 0xFFFFFFFF, _np(out))
    if n != 768:
        raise ValueError("only mode 1 has a TII table: %r" % (mode,))
    return out.reshape(4, 8, 24)


def tii_main_id(mask):
    """a comb's mask (bit b = group b) -> the main identifier p, 0 ... 69, or -1 if it is no pattern of one transmitter
    (not exactly four of the low 8 bits)"""
    m = int(mask)
    return -1 if m < 0 or m > 0xFFFFFFFF else int(lib().vit_tii_main_id(m))


def tii_records(words, ncombs):
    """a copied-back d_tii (numpy array of ngrp * (2 + 2*ncombs) 4-byte words) -> structured array (ngrp,) with the fields
    nused (uint32), noise (float32), comb (ncombs,) of mask (uint32) and strength (float32); a view, nothing is copied"""
    dt = np.dtype([("nused", "<u4"), ("noise", "<f4"), ("comb", [("mask", "<u4"), ("strength", "<f4")], (int(ncombs),))])
    w = np.ascontiguousarray(words).reshape(-1)
    if w.dtype.itemsize != 4 or w.size % (2 + 2 * int(ncombs)):
        raise ValueError("words must hold whole records of 2 + 2*ncombs 4-byte words")
    return w.view(dt)


def decode_stream_multi(d_symbols_u8, d_out, framebits, nframes, devices, chunk_frames, root_frames=-1, flags=0,
                        stream=None):
    """ONE process, several GPUs (include/viterbi_amd.h Part 3): the stream lives on devices[0]; synchronous."""
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    _check(lib().vit_decode_stream_multi(C.c_void_p(d_symbols_u8.data_ptr()), C.c_void_p(d_out.data_ptr()), framebits,
                                         nframes, devs, len(devices), chunk_frames, root_frames, flags,
                                         _stream_ptr(stream)), "vit_decode_stream_multi")


def make_descs(framebits_list, sym_align=4):
    """Contiguous layout for a variable-length batch -> (desc array, sym bytes, out bytes)."""
    fb = np.asarray(framebits_list, np.int64)
    sym_sz = 4 * (fb + TAIL)
    out_sz = (fb + 7) // 8
    d = np.zeros(fb.size, DESC_DTYPE)
    d["framebits"] = fb
    d["sym_offset"] = np.concatenate(([0], np.cumsum(sym_sz)[:-1]))
    d["out_offset"] = np.concatenate(([0], np.cumsum(out_sz)[:-1]))
    return d, int(sym_sz.sum()), int(out_sz.sum())
