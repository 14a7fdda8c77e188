"""Shared by tests/test_hinit_host.py and tests/test_gpu_hinit.py: a counted copy of the per-model example's FlatCluster restatement, the
pools the device launch is checked on, and the comparison of an estimated model with a reference's model files at the bars of
test_gpu_demo.py::test_hinit_viterbi_training / test_hinit_mixture_training."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
MIN_CLUST_SIZE, MAX_CLUST_ITER = 3, 10


def flat_cluster_counted(X, nc):
    """examples/hinit_model.py::flat_cluster, statement for statement, with the assignment returned and two counters: how often the
    repair loop perturbed the fullest cluster, and how many items ever had their minimum distance at two centres at once."""
    X = np.ascontiguousarray(X, np.float32)
    n, D = X.shape
    if n < nc:
        raise ValueError("InitClustering: only %d items for %d clusters" % (n, nc))
    f32 = np.float32
    cmap = np.zeros(n, np.int64)
    ctr = np.zeros((nc, D), f32); csize = np.zeros(nc, np.int64); ave = np.zeros(nc, f32)
    csize[0] = n; ave[0] = f32(1.0)
    count = dict(repairs=0, ties=0)

    def find_centres(k):
        for c in range(k):
            rows = X[cmap == c]
            tot = np.cumsum(rows, axis=0, dtype=f32)[-1] if rows.shape[0] else np.zeros(D, f32)
            with np.errstate(all="ignore"):
                ctr[c] = tot / f32(csize[c])

    def perturb(c, c2):
        v = ctr[c].copy()
        x = np.abs(v.astype(np.float64) * 0.01).astype(f32)
        x = np.where(x < f32(0.0001), f32(0.0001), x)
        ctr[c] = v + x; ctr[c2] = v - x

    def allocate(k):
        d = X[:, None, :] - ctr[None, :k, :]
        dist = np.sqrt(np.cumsum(d.astype(np.float64) ** 2, axis=2)[:, :, -1]).astype(f32)
        best = np.argmin(dist, axis=1)
        mn = dist[np.arange(n), best]
        count["ties"] += int(((dist == mn[:, None]).sum(axis=1) > 1).sum())
        total = np.cumsum(mn, dtype=f32)[-1]
        for c in range(k):
            sel = mn[best == c]
            csize[c] = sel.shape[0]
            ave[c] = np.cumsum(sel, dtype=f32)[-1] if sel.shape[0] else f32(0.0)
        cmap[:] = best
        for c in range(k):
            if csize[c] < MIN_CLUST_SIZE:
                return c + 1, total
            ave[c] = ave[c] / f32(csize[c])
        return 0, total

    find_centres(1)
    for c in range(2, nc + 1):
        big, mx = 0, ave[0]
        for k in range(1, c - 1):
            if ave[k] > mx:
                mx = ave[k]
                if csize[k] >= MIN_CLUST_SIZE:
                    big = k
        perturb(big, c - 1)
        old = f32(1e10)
        it = 0
        while True:
            repair = 0
            ce, new = allocate(c)
            while ce != 0:
                repair += 1
                if repair > c:
                    break
                full, mxs = 0, csize[0]
                for k in range(c):
                    if csize[k] > mxs:
                        mxs = csize[k]; full = k
                count["repairs"] += 1
                perturb(full, ce - 1)
                ce, new = allocate(c)
            if ce != 0:
                raise ValueError("FlatCluster: failed to make %d clusters" % c)
            converged = it >= MAX_CLUST_ITER or f32(f32(old - new) / old) < f32(0.001)
            find_centres(c); old = new
            it += 1
            if converged:
                break
    var = np.zeros((nc, D), f32)
    for c in range(nc):
        rows = X[cmap == c]
        d = (rows - ctr[c]).astype(np.float64)
        var[c] = (np.cumsum(d * d, axis=0)[-1] / float(csize[c])).astype(f32)
    return csize.copy(), ctr, var, cmap.copy(), count


def cluster_pools():
    """name -> (rows [n, D] float32, nc): the pools of the FlatCluster check, D = 39 unless the name says otherwise."""
    r = np.random.RandomState(20240611)
    blob = lambda n, D, k, spread=6.0: (r.randn(n, D) + spread * r.randn(k, D)[r.randint(0, k, n)]).astype(np.float32)
    pools = {}
    pools["one_cluster"] = (blob(7, 5, 1), 1)
    # exactly 3 nc items: four tight groups of three on a line
    g = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [80.0, 0.0, 0.0], [120.0, 0.0, 0.0]], np.float32)
    pools["three_per_cluster"] = ((np.repeat(g, 3, axis=0) + 0.1 * np.random.RandomState(7).randn(12, 3)).astype(np.float32), 4)
    pools["dim_1"] = (blob(41, 1, 3), 3)
    pools["dim_39"] = (blob(301, 39, 4), 4)
    # the mean is exactly 0, so the first split's centres are +-1e-4 and the item at 0 is as far from one as from the other
    k = np.arange(-4, 5, dtype=np.float32)
    pools["equidistant"] = (np.stack([k, -k], axis=1), 2)
    # near-duplicates in two tight groups: a split leaves a cluster under MIN_CLUST_SIZE and the fullest is perturbed again (seed 103);
    # the same recipe with seed 102 and four clusters cannot be split at all ("Failed to make 4 clusters")
    def dups(seed):
        q = np.random.RandomState(seed)
        dup = (1.0 + 1e-3 * q.randn(24, 4)).astype(np.float32)
        far = (3.0 + 1e-3 * q.randn(6, 4)).astype(np.float32)
        return np.concatenate([dup[:10], far[:3], dup[10:], far[3:]])
    pools["repair"] = (dups(103), 3)
    pools["cannot_split"] = (dups(102), 4)
    pools["many_39"] = (blob(997, 39, 16, 8.0), 16)
    return pools


def ref_trace(log_path, name):
    lines = [l for l in open(log_path) if l.startswith("HInit %s:" % name)]
    ref = [float(re.search(r"Average LogP = *(-?[\d.]+)", l).group(1)) for l in lines if "Average LogP" in l]
    return ref, any("converged" in l for l in lines)


def compare_model(p, q0, h, rq, rh, weights=False):
    """Parameters p of model h (layout q0) against the reference's set rq, model rh: the bars of test_hinit_viterbi_training (means within
    1e-4 of max(|mean|, sigma) + 1e-6, variances and linear transitions at rtol 1e-4 / atol 1e-7) and, with `weights`, weights within 1e-5."""
    for s, rs in zip(q0["hmmState"][q0["hmmStateOff"][h]:q0["hmmStateOff"][h + 1]], rq["hmmState"][rq["hmmStateOff"][rh]:rq["hmmStateOff"][rh + 1]]):
        c0, c1, r0, r1 = int(q0["stateCompOff"][s]), int(q0["stateCompOff"][s + 1]), int(rq["stateCompOff"][rs]), int(rq["stateCompOff"][rs + 1])
        assert c1 - c0 == r1 - r0
        for c, rc in zip(range(c0, c1), range(r0, r1)):
            g, rg = int(q0["compGauss"][c]), int(rq["compGauss"][rc])
            sigma = np.sqrt(rq["var"][rg])
            if weights:
                assert abs(p["compWeight"][c] - rq["compWeight"][rc]) <= 1e-5, (h, c, p["compWeight"][c], rq["compWeight"][rc])
            assert (np.abs(p["mean"][g] - rq["mean"][rg]) <= 1e-4 * np.maximum(np.abs(rq["mean"][rg]), sigma) + 1e-6).all(), (h, c)
            assert np.allclose(p["var"][g], rq["var"][rg], rtol=1e-4, atol=1e-7), (h, c)
    t, rt = int(q0["hmmTrans"][h]), int(rq["hmmTrans"][rh])
    N = int(q0["transN"][t])
    lin = lambda v: np.where(v > -0.5e10, np.exp(v.astype(np.float64)), 0.0)
    assert np.allclose(lin(p["transP"][q0["transOff"][t]:q0["transOff"][t] + N * N]), lin(rq["transP"][rq["transOff"][rt]:rq["transOff"][rt] + N * N]), rtol=1e-4, atol=1e-7), h


def model_params_equal(p, q, pk, h):
    """bit equality of model h's parameters in two parameter dicts of the same layout"""
    ok = True
    for s in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]:
        for c in range(int(pk["stateCompOff"][s]), int(pk["stateCompOff"][s + 1])):
            g = int(pk["compGauss"][c])
            ok = ok and np.array_equal(p["mean"][g], q["mean"][g]) and np.array_equal(p["var"][g], q["var"][g]) and p["compWeight"][c] == q["compWeight"][c]
    t = int(pk["hmmTrans"][h]); N = int(pk["transN"][t]); o = int(pk["transOff"][t])
    return bool(ok and np.array_equal(p["transP"][o:o + N * N], q["transP"][o:o + N * N]))
