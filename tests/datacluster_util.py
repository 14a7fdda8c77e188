"""Data-driven clustering (HHEd TC / NC / TI): the fixture tests/golden/datacluster (made by tests/golden/make_datacluster_golden.py) and
literal numpy / Python restatements of the reference's arithmetic, shared by the generator and the tests.

divergence_matrix performs the roundings of Divergence (HHEd.c:1749) one by one; ref_clustering is Clustering (:2005) + RemOutliers (:1975)
with SetGDist (:1818) recomputed in full after every merge -- no incremental bookkeeping of its own."""
import gzip
import os

import numpy as np

import treeclust_util as tu

ROOT = tu.ROOT
G = os.path.join(ROOT, "tests", "golden", "datacluster")
f32, f64 = np.float32, np.float64


def golden_bytes(name: str) -> bytes:
    p = os.path.join(G, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    return gzip.open(p + ".gz", "rb").read()


def divergence_matrix(mean, var):
    """float32[N, N]: StateDistance of single-Gaussian DIAGC states."""
    mean = np.asarray(mean, f32); var = np.asarray(var, f32)
    N, V = mean.shape
    s = np.zeros((N, N), f32)
    for k in range(V):
        x = (mean[:, None, k] - mean[None, :, k]).astype(f32)               # float subtract
        xx = (x * x).astype(f32)                                           # float multiply
        vv = (var[:, None, k] * var[None, :, k]).astype(f32)               # float multiply, then widened
        q = xx.astype(f64) / np.sqrt(vv.astype(f64))                       # double sqrt, double divide
        s = (s.astype(f64) + q).astype(f32)                                # double add, rounded to float
    d = np.sqrt((s / f32(V)).astype(f32).astype(f64)).astype(f32)          # float divide, double sqrt, rounded to float
    d = (f32(0.0) + d).astype(f32)
    np.fill_diagonal(d, 0.0)
    return d


def gdistance_matrix(scores, obs_off):
    """float32[N, N] from scores[obs, item] (SOutP of every component mean under every item): GDistance (:1771)."""
    N = len(obs_off) - 1
    d = np.zeros((N, N), f32)
    for i in range(N):
        for j in range(i + 1, N):
            s = f32(0.0)
            for o in range(obs_off[i], obs_off[i + 1]):
                s = f32(s + scores[o, j])
            for o in range(obs_off[j], obs_off[j + 1]):
                s = f32(s + scores[o, i])
            x = f32(f32(0.0) + f32(-(f32(s / f32(obs_off[j + 1] - obs_off[j])))))
            d[i, j] = d[j, i] = x
    return d


def set_gdist(cvec, idist):
    """SetGDist: every group distance from the item matrix, each maximum started at 0.0."""
    n, N = len(cvec), idist.shape[0]
    member = np.zeros((n, N), bool)
    for g, ch in enumerate(cvec):
        member[g, ch] = True
    rows = np.max(np.where(member[:, :, None], idist[None, :, :], -np.inf), axis=1)          # [group, item]
    gd = np.max(np.where(member[None, :, :], rows[:, None, :], -np.inf), axis=2)             # [group, group]
    gd = np.where(gd > 0.0, gd, 0.0).astype(f32)
    np.fill_diagonal(gd, 0.0)
    return gd


def min_gdist(g):
    """MinGDist: strict <, first pair in row-major order (1-based pair)."""
    n = g.shape[0]
    mn, mi, mj = g[0, 1], 1, 2
    for i in range(n - 1):
        row = g[i, i + 1:]
        j = int(np.argmin(row))                  # the first minimum of the row
        if row[j] < mn:
            mn, mi, mj = row[j], i + 1, i + 2 + j
    return mn, mi, mj


def ref_clustering(idist, num_req=1, threshold=1.0e15, occ=None, outlier=0.0):
    """(merge log [(i, j)] 1-based in the numbering current at each merge, the clusters' member chains 0-based, lower-slot outlier merges)."""
    idist = np.asarray(idist, f32)
    N = idist.shape[0]
    cvec = [[i] for i in range(N)]
    g = idist.copy()
    log, lower = [], 0
    threshold = f32(threshold)
    if N >= 2:
        mn, i, j = min_gdist(g)
        while len(cvec) > num_req and mn < threshold:
            cvec[i - 1] = cvec[i - 1] + cvec[j - 1]; del cvec[j - 1]
            log.append((i, j))
            g = set_gdist(cvec, idist)
            if len(cvec) < 2:
                break
            mn, i, j = min_gdist(g)
    if occ is not None:
        occ = np.asarray(occ, f32)
        sums = []
        for ch in cvec:
            s = f32(0.0)
            for m in ch:
                s = f32(s + occ[m])
            sums.append(s)
        outlier = f32(outlier)
        while len(cvec) > 1:
            sp = int(np.argmin(np.array(sums, f32)))                   # MinOccSum: the first minimum
            if not sums[sp] < outlier:
                break
            row = g[sp].copy(); row[sp] = np.inf
            cand = [k for k in range(len(cvec)) if k != sp]
            mini = cand[int(np.argmin(np.array([g[sp, k] for k in cand], f32)))]
            cvec[sp] = cvec[sp] + cvec[mini]; sums[sp] = f32(sums[sp] + sums[mini])
            log.append((sp + 1, mini + 1))
            lower += mini < sp
            del cvec[mini]; del sums[mini]
            g = set_gdist(cvec, idist)
    return log, cvec, lower


def replay(N, log):
    cvec = [[i] for i in range(N)]
    for i, j in log:
        cvec[i - 1] = cvec[i - 1] + cvec[j - 1]; del cvec[j - 1]
    return cvec
