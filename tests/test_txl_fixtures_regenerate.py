"""The committed TXL rep-net fixtures (tests/golden/txl/*.npz) are what the reference's code produces today:
``scripts/make_golden_txl.py`` regenerates them into a temporary directory (development container only: it needs the
reference checkout) and every array must match -- integers and flags bit for bit, floats to 1e-6 of the array's largest
value."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX = os.path.join(ROOT, "tests", "golden", "txl")
REFERENCE = "/root/reference/SubgraphCountingMatching"


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference checkout (development container only)")
def test_committed_txl_fixtures_equal_a_fresh_run_of_the_reference(tmp_path):
    env = dict(os.environ, DMP_GOLDEN_TXL_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_golden_txl.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    have = sorted(f for f in os.listdir(TX) if f.endswith(".npz"))
    assert fresh == have, sorted(set(fresh) ^ set(have))
    for f in have:
        with np.load(os.path.join(TX, f), allow_pickle=False) as a, np.load(os.path.join(tmp_path, f), allow_pickle=False) as b:
            assert sorted(a.files) == sorted(b.files), f
            for k in a.files:
                x, y = a[k], b[k]
                assert x.shape == y.shape and x.dtype == y.dtype, (f, k)
                if x.dtype.kind in "fc":
                    if x.size:
                        scale = max(1.0, float(np.abs(x).max()))
                        assert float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) <= 1e-6 * scale, (f, k)
                else:
                    assert x.tobytes() == y.tobytes(), (f, k)
