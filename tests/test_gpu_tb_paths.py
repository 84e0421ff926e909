"""GPU: every path of the block-parallel tracebacks (csrc/vit_pk.hip: traceback_part16, its in-flight <SPEC> form and the
chain loop of vit_pk_long_kernel, traceback_part; csrc/vit_lat.hip) with the merge-directed frames of tests/tbdirect.py -
frames kept because a model of the traceback says which block misses, how deep the re-trace cascade runs, which in-flight
part fails its check and where the wave gives up (class counts: tests/test_tb_paths_host.py, on the CPU).

Everything goes through the C ABI; outputs start as a sentinel with 64 guard bytes on both sides; every byte is compared
with the oracle.  The path counters of the -DVIT_DIAG_SPEC build are compared with the models' totals in a child process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before libviterbi.so is loaded: a run of this module alone must bring up torch's HIP runtime first

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tbdirect as D  # noqa: E402

GUARD, SENTINEL = 64, 0xA5


class Want:
    """the oracle's bytes per distinct frame and comparator, computed once"""

    def __init__(self, O):
        self.O, self.sym, self.out = O, {}, {}

    def symbols(self, sp):
        if sp.key() not in self.sym:
            self.sym[sp.key()] = sp.symbols()
        return self.sym[sp.key()]

    def bytes(self, sp, ge):
        k = (sp.key(), bool(ge))
        if k not in self.out:
            self.out[k] = self.O.decode_batch(sp.fb, self.symbols(sp), ge=bool(ge))[0]
        return self.out[k]


@pytest.fixture(scope="module")
def want(O):
    return Want(O)


@pytest.fixture(scope="module")
def directed():
    waves, lat = D.load_directed()
    return waves, lat, D.batches(waves)


def _launch(V, torch, specs, want, kernel, ge, entry, u32=False):
    """one launch over the frames -> nothing; asserts guards and every frame's bytes.  entry: "uniform" | "desc\""""
    lens = [s.fb for s in specs]
    sym = np.concatenate([want.symbols(s) for s in specs])
    exp = np.concatenate([want.bytes(s, ge) for s in specs])
    d_out = torch.full((exp.size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(1 if ge else 0)
    try:
        if entry == "uniform":
            assert len(set(lens)) == 1
            if u32:
                V.decode_batch_dev_u32(torch.from_numpy(sym.astype(np.uint32)).cuda(), d_out[GUARD:], lens[0], len(lens))
            else:
                V.decode_batch_dev(torch.from_numpy(sym).cuda(), d_out[GUARD:], lens[0], len(lens))
        else:
            desc, _, _ = V.make_descs(lens)
            V.decode_varlen_dev(torch.from_numpy(sym).cuda(), d_out[GUARD:], torch.from_numpy(desc.view(np.uint8)).cuda(),
                                len(lens), max(lens))
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)
    got = d_out.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + exp.size:] == SENTINEL).all(), "wrote outside the output"
    got = got[GUARD:GUARD + exp.size]
    if not np.array_equal(got, exp):
        at = np.cumsum([0] + [(fb + 7) // 8 for fb in lens])
        bad = [(i, specs[i].key()) for i in range(len(specs)) if not np.array_equal(got[at[i]:at[i + 1]], exp[at[i]:at[i + 1]])]
        pytest.fail("kernel %d ge %d %s%s: %d of %d frames differ from the oracle, first (index, recipe): %s" % (
            kernel, ge, entry, " u32" if u32 else "", len(bad), len(specs), bad[:4]))


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_directed_batches(V, torch_cuda, want, directed, kernel, ge):
    """every directed wave, in the launch whose waves the models describe (uniform entry per length; descriptor tables of
    three waves, which the device does not sort) and, for the uniform batches, through a descriptor table as well (sixteen
    frames and more: sorted on the device - the waves regroup, the bytes must not change)"""
    _, _, batches = directed
    for b in batches:
        if b.framebits is not None:
            _launch(V, torch_cuda, b.specs, want, kernel, ge, "uniform")
        _launch(V, torch_cuda, b.specs, want, kernel, ge, "desc")


@pytest.mark.parametrize("kernel", [0, 2, 3])
def test_u32_entry(V, torch_cuda, want, directed, kernel):
    """vit_decode_batch_dev_u32 (narrowing fused into the symbol loads): one short, the in-flight and the longest batch"""
    _, _, batches = directed
    for b in batches:
        if b.framebits in (768, 1024, 3200, 9216):
            _launch(V, torch_cuda, b.specs, want, kernel, 0, "uniform", u32=True)


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_latency_frames(V, torch_cuda, want, directed, kernel, ge):
    """the latency kernel's directed frames (BL = 6, 12, 144; lane 0, the top speculative lane, cascades to depth 30): one
    frame per launch as deconvolve() would send it, and all frames of a length together"""
    _, lat, _ = directed
    by_fb = {}
    for sp in lat:
        _launch(V, torch_cuda, [sp], want, kernel, ge, "uniform")
        by_fb.setdefault(sp.fb, []).append(sp)
    for fb, specs in by_fb.items():
        _launch(V, torch_cuda, specs, want, kernel, ge, "uniform")
    _launch(V, torch_cuda, lat, want, kernel, ge, "desc")


def _uniform_random_spec(fb, k):
    return D.Spec(fb, 7000 + k, None, [("uniform", fb + D.TAIL, fb + D.TAIL)])  # the whole frame overwritten with uniform bytes


def test_wave_company(V, torch_cuda, want, directed):
    """each directed frame of the fast and in-flight forms in each of the four slots of its wave, beside three clean
    frames, three frames of uniform random bytes (each slot gives up, re-traces and cascades on its own) and three other
    directed frames; the general-form waves with their four lengths rotated through the slots.  Packed kernel."""
    waves, _, _ = directed
    by_fb = {}
    for w in waves:
        if w.entry == "uniform":
            by_fb.setdefault(w.specs[0].fb, [])
            for sp in w.specs:
                if sp.bursts and sp.key() not in {s.key() for s in by_fb[sp.fb]}:
                    by_fb[sp.fb].append(sp)
    for fb, ds in sorted(by_fb.items()):
        specs = []
        for i, sp in enumerate(ds):
            others = [ds[(i + j) % len(ds)] for j in (1, 2, 3)]
            for company in ([D.clean_spec(fb, k) for k in range(3)], [_uniform_random_spec(fb, k) for k in range(3)], others):
                for slot in range(4):
                    wave = list(company)
                    wave.insert(slot, sp)
                    specs += wave
        _launch(V, torch_cuda, specs, want, 2, 0, "uniform")
    cur = []
    for w in [w for w in waves if w.entry == "desc" and None not in w.specs and len({s.fb for s in w.specs}) > 1]:
        for rot in range(4):
            cur += w.specs[rot:] + w.specs[:rot]
            if len(cur) == 12:  # three waves: below the device sort's threshold, the table is consumed as listed
                _launch(V, torch_cuda, cur, want, 2, 0, "desc")
                cur = []
    if cur:
        _launch(V, torch_cuda, cur, want, 2, 0, "desc")


def test_one_large_batch(V, torch_cuda, want, directed):
    """the 3072-bit directed waves tiled to more groups than the long-frame kernel has persistent workgroups: the later
    groups of a workgroup (spill slice, window and carry reused) must decode what its first group would"""
    torch = torch_cuda
    _, _, batches = directed
    b = next(b for b in batches if b.framebits == 3072)
    props = torch.cuda.get_device_properties(0)
    groups_resident = 16 * props.multi_processor_count
    n0 = len(b.specs)
    tiles = (groups_resident * 4 * 9 // 4) // n0 + 1  # two and a quarter rounds
    sym = torch.from_numpy(np.stack([want.symbols(s) for s in b.specs])).cuda()
    exp = torch.from_numpy(np.stack([want.bytes(s, 0) for s in b.specs])).cuda()
    d_sym = sym.repeat(tiles, 1)
    d_out = torch.full((tiles * n0 * (3072 // 8) + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    old, old_ge = V.set_kernel(2), V.set_renorm_ge(0)
    try:
        V.decode_batch_dev(d_sym, d_out[GUARD:], 3072, tiles * n0)
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)
    assert tiles * n0 > 2 * 4 * groups_resident
    assert bool((d_out[:GUARD] == SENTINEL).all()) and bool((d_out[-GUARD:] == SENTINEL).all())
    same = (d_out[GUARD:-GUARD].view(tiles, n0, -1) == exp.unsqueeze(0)).all(dim=2)
    assert bool(same.all()), "tiles x frames that differ: %s" % same.logical_not().nonzero()[:8].tolist()


def test_diag_counters_equal_the_models(V):
    """the -DVIT_DIAG_SPEC build (libviterbi_diag.so, made by build()) in a fresh process: groups, parts traced in flight,
    give-ups, parts traced after the forward pass, failed checks, fast-form pass-0 misses, fast-form passes and switches
    to the long warm-up, per directed batch and comparator, must EQUAL the models' totals; the bytes the oracle's.  This is
    what catches a change that moves work between paths without changing a byte (a give-up at > 8 instead of >= 8)."""
    diag = os.path.join(os.path.dirname(V.LIB_PATH), "libviterbi_diag.so")  # next to the library under test
    assert os.path.exists(diag), "libviterbi_diag.so is missing: __graft_entry__.build() makes it"
    env = dict(os.environ, VITERBI_AMD_LIB=diag)
    r = subprocess.run([sys.executable, os.path.join(HERE, "tb_diag_child.py")], env=env, capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.startswith("ok ")]
    assert r.returncode == 0 and not bad and len(lines) >= 2 * 20, "%s\n%s" % ("\n".join(bad[:8] or lines[-8:]), r.stderr[-2000:])
