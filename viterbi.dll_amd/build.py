"""Build libviterbi.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libviterbi.so")
SOURCES = ["vit_api.hip", "vit_ring.hip", "vit_api_decode.hip", "vit_api_ens.hip", "vit_api_ofdm.hip", "vit_wave.hip", "vit_pk.hip", "vit_sort.hip", "rs_kernels.hip", "rs_table.hip", "vit_multi.hip", "vit_lat.hip",
           "vit_punct.hip", "vit_dab.hip", "vit_ti.hip", "vit_ofdm.hip", "vit_ofdm_td.hip", "vit_ofdm_sync.hip",
           "vit_iq_convert.hip", "vit_ofdm_acq.hip", "vit_ofdm_tii.hip", "vit_resample.hip", "vit_packet.hip", "vit_packet_table.hip", "vit_dgroup.hip", "vit_dgroup_table.hip", "vit_api_packet.hip",
           "vit_mci.hip", "vit_mci_dir.hip", "vit_api_mci.hip"]
PK8_SOURCE = "vit_pk8.hip"  # round-3 experiment (8 frames per wavefront, slower): only with extra=["-DVIT_WITH_PK8"]
DEPS = SOURCES + ["vit_internal.h", "vit_host.h", "rs_dev.h", "vit_pk_dev.h", "vit_pk_acs.h", "vit_pk_tb.h", "vit_pk_fixed.h", "vit_pk_long.h", "vit_punct_dev.h", "vit_fft_dev.h", "vit_iq_dev.h", "vit_csi_dev.h", "vit_demap_dev.h", "vit_wave_dev.h", "vit_crc_dev.h", "vit_packet_fmt.h", "vit_packet_dev.h", "vit_dgroup_dev.h", "vit_fec_block.inc","vit_image_dev.h", "vit_fig_fmt.h", "vit_fib_group_dev.h", "exports.map"]


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, d) for d in DEPS] + [os.path.join(ROOT, "include", "viterbi_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra=(), out=None):
    """extra/out: kernel experiments (tools/exp/ab.sh) build flag variants next to the product library"""
    if out is None and not force and not _stale():
        return SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-Wall", "-Wno-unused-function",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"),
           "-o", out or SO] + list(extra) + [os.path.join(CSRC, s) for s in SOURCES + ([PK8_SOURCE] if "-DVIT_WITH_PK8" in extra else [])] + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out or SO


if __name__ == "__main__":
    build(force="-f" in sys.argv, verbose=True)
    print(SO)
