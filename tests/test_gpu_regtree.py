"""Regression class trees (HHEd RC) on the device: the library's .tree and .base files against HHEd's recorded ones, byte for byte
(tests/golden/regtree, written by tests/golden/make_regtree_golden.py; the cases are described in tests/regtree_util.py: CASES), and
-- where the reference's HHEd binary is at hand -- a sweep of seeded random sets against the binary itself."""
import json
import os

import numpy as np
import pytest

import regtree_util as ru

pytestmark = pytest.mark.gpu


def _same_files(got_dir, ref_dir):
    for f in ("rtree.tree", "rtree.base"):
        got, ref = open(os.path.join(str(got_dir), f), "rb").read(), open(os.path.join(str(ref_dir), f), "rb").read()
        assert got == ref, f


@pytest.mark.parametrize("name", sorted(ru.CASES))
def test_files_equal_hhed(name, tmp_path):
    d = os.path.join(ru.GOLDEN, name)
    t = ru.run_library(d, tmp_path)
    iters, ms = t.stats()
    print("case %s: CalcDistance calls per split %s, kernels %.3f ms" % (name, iters, ms))
    _same_files(tmp_path, d)
    assert iters == json.load(open(os.path.join(ru.GOLDEN, "iterations.json")))[name]      # HHEd's own trace
    if name == "h":
        assert max(iters) > 10


def test_live_sweep_against_hhed(tmp_path):
    if not os.path.exists(ru.HHED):
        pytest.skip("oracle/_ref/HHEd is not built here")
    rng = np.random.RandomState(2024)
    for k in range(12):
        D = int(rng.randint(2, 8))
        H, S, M = int(rng.randint(4, 12)), int(rng.randint(2, 5)), int(rng.randint(1, 5))
        sil = bool(k % 3 == 0) and H * S * M - S * M > 3 * D
        d = tmp_path / ("s%02d" % k)
        ru.write_set(str(d), ru.names_for(H, sil=sil), S, M, D, seed=100 + k, occ_zero=((1, 0),) if k % 4 == 1 else (), tied=(k % 4 == 2 and M >= 2 and S >= 2),
                     clusters=3 if k % 2 else 0)
        ru.write_script(str(d), int(rng.randint(2, 12)), "{sil.state[2-%d].mix}" % (S + 1) if sil else None)
        ru.run_hhed(str(d))
        out = d / "lib"
        out.mkdir()
        t = ru.run_library(str(d), out)
        print("set %d: D=%d %dx%dx%d sil=%s -> %d nodes, iterations %s" % (k, D, H, S, M, sil, t.num_nodes, t.stats()[0]))
        _same_files(out, d)
    # the shapes of tests/test_gpu_regtree_kernels.py end to end: more members than the workgroup has threads, the project's vector size,
    # dimension lanes over two wavefronts, and zero occupations beside shared states and Gaussians.  Each has G > 3 D, so that a split happens.
    for tag, H, S, M, D, n_term, more in (("g1120", 70, 4, 4, 3, 16, dict(clusters=4)), ("d39", 15, 3, 4, 39, 4, {}), ("d65", 15, 3, 6, 65, 4, dict(clusters=3)),
                                          ("zt", 8, 3, 3, 4, 6, dict(occ_zero=((1, 0), (3, 2)), tied=True))):
        d = tmp_path / tag
        ru.write_set(str(d), ru.names_for(H), S, M, D, seed=300 + D, **more)
        ru.write_script(str(d), n_term)
        ru.run_hhed(str(d))
        out = d / "lib"
        out.mkdir()
        t = ru.run_library(str(d), out)
        print("set %s: D=%d %dx%dx%d -> %d nodes, iterations %s" % (tag, D, H, S, M, t.num_nodes, t.stats()[0]))
        assert t.num_nodes >= 3
        _same_files(out, d)
