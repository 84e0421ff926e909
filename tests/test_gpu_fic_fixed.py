"""GPU: the fixed-geometry instantiation of the packed kernel (csrc/vit_pk.hip: vit_pk_fixed_kernel, taken by vit_launch_pk
for a uniform batch of 768-bit frames) - what only its dispatch and its compile-time geometry can get wrong.  The launches
live in tests/fic_fixed_cases.py: batch sizes around a group of four and around one round of waves (the switch to the
rotating-priority instantiation), both ingest formats, the lengths next to 768 and the descriptor-table entry (which stay
on the general kernel), and the input families (Eb/N0 3 dB, uniform random bytes, saturation / renormalisation stress,
hard decisions), 256 distinct frames tiled.

Through the C ABI; outputs pre-filled with a sentinel, guard bytes on both sides; every byte compared with the oracle in both
comparator modes.  The same launches run once more in a child process on libviterbi_general.so, the library built with
-DVIT_FIC_FIXED=0 (made by build()), so that the general kernel keeps its coverage at 768 bits.
"""
import os
import subprocess
import sys

import pytest
import torch  # noqa: F401  before libviterbi.so is loaded: a run of this module alone must bring up torch's HIP runtime first

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fic_fixed_cases as F  # noqa: E402


@pytest.fixture(scope="module")
def data(O):
    return F.Data(O)


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("case", sorted(F.CASES))
def test_fic_fixed(V, torch_cuda, data, case, ge):
    msgs = [m for m in F.CASES[case](V, torch_cuda, data, ge) if m]
    assert not msgs, "\n".join(msgs)


def test_same_launches_without_the_fixed_instantiation(V):
    """libviterbi_general.so (-DVIT_FIC_FIXED=0) in a fresh process: every case above on the general kernel"""
    lib = os.path.join(os.path.dirname(V.LIB_PATH), "libviterbi_general.so")  # next to the library under test
    assert os.path.exists(lib), "libviterbi_general.so is missing: __graft_entry__.build() makes it"
    env = dict(os.environ, VITERBI_AMD_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(HERE, "fic_fixed_cases.py")], env=env, capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.startswith("ok ")]
    assert r.returncode == 0 and not bad and len(lines) == 2 * len(F.CASES), "%s\n%s" % ("\n".join(bad[:8] or lines[-8:]), r.stderr[-2000:])
