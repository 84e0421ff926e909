"""The launches of tests/test_gpu_fic_fixed.py, kept apart from pytest so that the same launches can run in a child process on
the library built WITHOUT the fixed-geometry instantiation (-DVIT_FIC_FIXED=0, libviterbi_general.so): what the dispatch in
vit_launch_pk and the fixed geometry of vit_pk_fixed_kernel (csrc/vit_pk.hip) can get wrong - group and round boundaries, both
ingest formats, the lengths and entries next to 768 bits that must stay on the general kernel, and the input families.

Everything goes through the C ABI; outputs start as a sentinel with guard bytes on both sides; every byte is compared with the
oracle in both comparator modes.  As a script: runs every case on the library in VITERBI_AMD_LIB, prints one line per case,
exit status 0 only if all agree.
"""
import os
import sys

import numpy as np

FB = 768
GUARD, SENTINEL = 64, 0xA5
BASE_N = 256


class Data:
    """256 distinct frames per input family and the oracle's bytes per comparator, computed once"""

    def __init__(self, O):
        self.O, self._sym, self._want = O, {}, {}

    def _make(self, fam, fb):
        O, n, sl = self.O, BASE_N, self.O.sym_len(fb)
        if fam == "3db":
            return O.noisy_frames(n, fb, seed=fb + 31)
        if fam == "random":  # no signal: half of the 30-step speculations miss, many re-trace passes
            return O.uniform_symbols(n * sl, seed=fb + 32).reshape(n, sl)
        if fam == "stress":  # the 255 clamp and the subs-63 floor (as tests/test_gpu_parity.py builds them)
            rng = np.random.default_rng(11)
            sym = np.empty((n, sl), np.uint8)
            sym[0::4] = 0
            sym[1::4] = 255
            sym[2::4] = rng.integers(0, 2, (n // 4, sl), dtype=np.uint8) * 255
            blk = rng.integers(0, 256, (n // 4, sl // 64 + 1), dtype=np.uint8)
            sym[3::4] = np.repeat(blk, 64, axis=1)[:, :sl]
            return sym
        if fam == "hard":  # the families on which the two renormalise comparators differ
            return np.concatenate([O.hard_random_symbols(n // 2, fb, seed=fb + 33),
                                   O.hard_flipped_frames(n // 2, fb, flip=0.2, seed=fb + 34)])
        if fam == "mixed":
            return np.concatenate([self.sym(f, fb)[:n // 4] for f in ("3db", "random", "stress", "hard")])
        raise KeyError(fam)

    def sym(self, fam, fb=FB):
        if (fam, fb) not in self._sym:
            self._sym[fam, fb] = np.ascontiguousarray(self._make(fam, fb))
        return self._sym[fam, fb]

    def want(self, fam, ge, fb=FB):
        k = (fam, fb, bool(ge))
        if k not in self._want:
            self._want[k] = self.O.decode_batch(fb, self.sym(fam, fb), nthreads=8, ge=bool(ge))
        return self._want[k]


def launch(V, torch, data, fam, n, ge, fb=FB, kernel=2, u32=False, entry="uniform"):
    """n frames = the family's 256 tiled and cut; the symbol buffer ends with the last frame's last symbol, the output has
    guard bytes on both sides.  Compares on the device, tile by tile.  -> None or a message"""
    nb = (fb + 7) // 8  # a partial last byte is padded with zero bits
    d_base = torch.from_numpy(data.sym(fam, fb)).cuda()
    reps = (n + BASE_N - 1) // BASE_N
    d_sym = d_base.repeat(reps, 1)[:n].contiguous()
    if u32:
        # only the low byte of a symbol counts (the reference ABI's format): junk above it
        d_sym = d_sym.to(torch.int32) | (torch.arange(d_sym.numel(), device="cuda", dtype=torch.int32).view_as(d_sym) << 8)
    d_want = torch.from_numpy(data.want(fam, ge, fb)).cuda().repeat(reps, 1)[:n]
    d_out = torch.full((n * nb + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(1 if ge else 0)
    try:
        if entry == "desc":
            desc, sym_bytes, out_bytes = V.make_descs([fb] * n)
            assert sym_bytes == d_sym.numel() and out_bytes == n * nb and not u32
            V.decode_varlen_dev(d_sym.view(-1), d_out[GUARD:], torch.from_numpy(desc.view(np.uint8)).cuda(), n, fb)
        elif u32:
            V.decode_batch_dev_u32(d_sym, d_out[GUARD:], fb, n)
        else:
            V.decode_batch_dev(d_sym, d_out[GUARD:], fb, n)
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)
    if not (bool((d_out[:GUARD] == SENTINEL).all()) and bool((d_out[GUARD + n * nb:] == SENTINEL).all())):
        return "wrote outside the output (%s, n=%d)" % (fam, n)
    bad = (d_out[GUARD:GUARD + n * nb].view(n, nb) != d_want).any(dim=1)
    if bool(bad.any()):
        return "%s fb=%d n=%d ge=%d kernel=%d%s %s: %d frames differ from the oracle, first %s" % (
            fam, fb, n, ge, kernel, " u32" if u32 else "", entry, int(bad.sum()), bad.nonzero()[:6].view(-1).tolist())
    return None


def _resident_groups(torch):
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count  # 10 KB of LDS per workgroup: 16 per CU


def case_group_sizes(V, torch, data, ge):
    """batches around one group of four: the missing frames of the last group read no symbols and write no bytes"""
    return [launch(V, torch, data, "mixed", n, ge) for n in (1, 3, 4, 5, 4095)]


def case_one_round(V, torch, data, ge):
    """one round of waves with more than one wave per SIMD (rotating priorities), forced and chosen"""
    return [launch(V, torch, data, "mixed", 8192, ge, kernel=k) for k in (2, 0)]


def case_just_over_one_round(V, torch, data, ge):
    """three groups more than the device holds at once (static priorities again), the last one ragged; and exactly one round"""
    g = _resident_groups(torch)
    return [launch(V, torch, data, "mixed", 4 * (g + 3) - 1, ge), launch(V, torch, data, "mixed", 4 * g, ge)]


def case_u32(V, torch, data, ge):
    """the reference ABI's u32 symbols read in place"""
    return [launch(V, torch, data, "mixed", n, ge, u32=True) for n in (5, 4095)]


def case_neighbours(V, torch, data, ge):
    """what must stay on the general kernel: the lengths next to 768 and a descriptor table of 768-bit frames (short: consumed
    as listed; from sixteen frames: sorted on the device)"""
    r = [launch(V, torch, data, "3db", 13, ge, fb=fb) for fb in (752, 770, 778)]
    return r + [launch(V, torch, data, "mixed", n, ge, entry="desc") for n in (7, 203)]


def _family(fam):
    def case(V, torch, data, ge):
        return [launch(V, torch, data, fam, 4 * BASE_N - 1, ge)]
    case.__doc__ = "input family %s, 256 distinct frames tiled" % fam
    return case


CASES = {"group_sizes": case_group_sizes, "one_round": case_one_round, "just_over_one_round": case_just_over_one_round,
         "u32": case_u32, "neighbours": case_neighbours, "family_3db": _family("3db"), "family_random": _family("random"),
         "family_stress": _family("stress"), "family_hard": _family("hard")}


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here)]
    import torch
    import _vitpkg
    V, O = _vitpkg.load_package(), _vitpkg.load_oracle()
    assert os.path.basename(V.LIB_PATH) == "libviterbi_general.so", V.LIB_PATH
    assert torch.cuda.is_available()
    V.initialize()
    data, bad = Data(O), 0
    for name, case in CASES.items():
        for ge in (0, 1):
            msgs = [m for m in case(V, torch, data, ge) if m]
            bad += bool(msgs)
            print("%s %s ge=%d %s" % ("FAIL" if msgs else "ok  ", name, ge, "; ".join(msgs)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
