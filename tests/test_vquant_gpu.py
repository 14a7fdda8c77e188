"""VQ codebooks and VQ coding on the device (csrc/vquant.hip) against plain numpy restatements of HTrain.c's FlatCluster / TreeCluster
and HVQ.c's GetVQ: float32 differences, float64 sums, float32 accumulators in item order -- compared bit for bit."""
import functools
import os

import numpy as np
import pytest

from htk_amd import capi

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vq")
NULLC, DIAGC, INVDIAGC, FULLC = capi.CK_NULLC, capi.CK_DIAGC, capi.CK_INVDIAGC, capi.CK_FULLC
f32, f64 = np.float32, np.float64


def seqsum(a):
    """The sum down axis 0 in order, in a's own type (np.sum adds pairwise)."""
    return np.add.accumulate(a, axis=0)[-1]


def tri(i, j):
    return i * (i + 1) // 2 + j


def distance(X, C, kind, cov):
    """Distance (HTrain.c:424) of every row of X to every row of C."""
    D = X.shape[1]
    s = np.zeros((len(X), len(C)), f64)
    if kind == FULLC:
        df = X[:, None, :] - C[None, :, :]
        for i in range(1, D):
            for j in range(i):
                s += (df[:, :, i] * df[:, :, j] * cov[tri(i, j)]).astype(f64)
        s *= 2
        for i in range(D):
            s += (df[:, :, i] * df[:, :, i] * cov[tri(i, i)]).astype(f64)
    else:
        for d in range(D):
            x = (X[:, None, d] - C[None, :, d]).astype(f64)
            q = x * x
            s += q / f64(cov[d]) if kind == DIAGC else q * f64(cov[d]) if kind == INVDIAGC else q
    return np.sqrt(s).astype(f32)


def perturb_step(v):
    x = np.abs(v.astype(f64) * 0.01).astype(f32)
    return np.where(x.astype(f64) < 0.0001, f32(0.0001), x)


def cov_invert(t, D):
    """CovInvert (HMath.c:567) of a packed lower triangle, every sum in its order."""
    L = np.zeros((D, D))
    for i in range(D):
        for j in range(i + 1):
            s = f64(t[tri(i, j)])
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    inv = np.zeros(D * (D + 1) // 2, f32)
    for i in range(D):
        y, x = np.zeros(D), np.zeros(D)
        y[i] = 1.0 / L[i, i]
        for j in range(i + 1, D):
            s = 0.0
            for k in range(i, j):
                s -= L[j, k] * y[k]
            y[j] = s / L[j, j]
        x[D - 1] = y[D - 1] / L[D - 1, D - 1]
        for j in range(D - 2, -1, -1):
            s = y[j]
            for k in range(j + 1, D):
                s -= L[k, j] * x[k]
            x[j] = s / L[j, j]
        for j in range(i, D):
            inv[tri(j, i)] = x[j]
    return inv


def find_covariance(X, idx, mean, kind):
    D = X.shape[1]
    x = (X[idx] - mean).astype(f64)
    nx = f64(len(idx))
    if kind == FULLC:
        t = np.array([seqsum(x[:, j] * x[:, k]) / nx for j in range(D) for k in range(j + 1)]).astype(f32)
        return cov_invert(t, D)
    sq = seqsum(x * x)
    return (sq / nx if kind == DIAGC else nx / sq).astype(f32)


def centre(X, idx):
    return seqsum(X[idx]) / f32(len(idx))


def ref_flat(X, nc, kind, cov, min_clust=3, max_iter=10):
    """FlatCluster (HTrain.c:763).  Returns the cluster set, or the reference's error number; `facts` counts the ties of the strict
    minimum and the repairs that fired."""
    N, D = X.shape
    facts = dict(ties=0, repairs=0)
    if N < nc:
        return 7120, facts
    ctr, ave, size = np.zeros((nc, D), f32), np.zeros(nc, f32), np.zeros(nc, np.int64)
    cmap = np.zeros(N, np.int64)
    size[0], ave[0] = N, 1.0
    ctr[0] = centre(X, np.arange(N))
    for c in range(2, nc + 1):
        mx, big = ave[0], 0
        for k in range(1, c - 1):                       # BiggestCluster, with its quirk
            if ave[k] > mx:
                mx = ave[k]
                if size[k] >= min_clust:
                    big = k
        x = perturb_step(ctr[big])
        ctr[c - 1] = ctr[big] - x
        ctr[big] = ctr[big] + x
        old, it = f32(1e10), 0
        while True:
            repair = 0
            while True:
                d = distance(X, ctr[:c], kind, cov)
                cmap = np.argmin(d, axis=1)
                mn = d[np.arange(N), cmap]
                facts["ties"] += int(((d == mn[:, None]).sum(1) > 1).sum())
                total, ce = seqsum(mn), 0
                for k in range(c):
                    idx = np.nonzero(cmap == k)[0]
                    size[k] = len(idx)
                    ave[k] = seqsum(mn[idx]) if len(idx) else 0.0
                for k in range(c):
                    if size[k] < min_clust:
                        ce = k + 1
                        break
                    ave[k] = ave[k] / f32(size[k])
                repair += 1
                if ce == 0 or repair > c:
                    break
                facts["repairs"] += 1
                full = int(np.argmax(size[:c]))
                x = perturb_step(ctr[full])
                if full == ce - 1:
                    ctr[full] = (ctr[full] + x) - x
                else:
                    ctr[ce - 1] = ctr[full] - x
                    ctr[full] = ctr[full] + x
            if ce:
                return 7120, facts
            with np.errstate(invalid="ignore"):            # (0 / 0 where every item is its own centre: not below the threshold)
                conv = it >= max_iter or f64((old - total) / old) < 0.001
            for k in range(c):
                ctr[k] = centre(X, np.nonzero(cmap == k)[0])
            old = total
            if conv:
                break
            it += 1
    covs = None if kind == NULLC else np.stack([find_covariance(X, np.nonzero(cmap == k)[0], ctr[k], kind) for k in range(nc)])
    return dict(size=size, centre=ctr, cov=covs, aveCost=ave, cmap=cmap), facts


def ref_tree(X, nc, kind, cov):
    """TreeCluster (HTrain.c:806), nodes numbered from 0."""
    N, D = X.shape
    if N < nc:
        return 7120
    nodes = 2 * nc - 1
    ctr, size, cmap = np.zeros((nodes, D), f32), np.zeros(nodes, np.int64), np.zeros(N, np.int64)
    covs = None if kind == NULLC else np.zeros((nodes, len(cov)), f32)
    size[0] = N
    ctr[0] = centre(X, np.arange(N))
    if covs is not None:
        covs[0] = find_covariance(X, np.arange(N), ctr[0], kind)
    row0, rows = 0, 1
    while rows < nc:
        for n in range(row0, row0 + rows):
            n1 = row0 + rows + 2 * (n - row0)
            x = perturb_step(ctr[n])
            ctr[n1], ctr[n1 + 1] = ctr[n] + x, ctr[n] - x
            idx = np.nonzero(cmap == n)[0]
            d = distance(X[idx], ctr[n1:n1 + 2], kind, cov)
            cmap[idx] = np.where(d[:, 0] < d[:, 1], n1, n1 + 1)
            for k in (n1, n1 + 1):
                ik = np.nonzero(cmap == k)[0]
                size[k] = len(ik)
                if len(ik) == 0:
                    return 7120
                ctr[k] = centre(X, ik)
                if covs is not None:
                    covs[k] = find_covariance(X, ik, ctr[k], kind)
        row0, rows = row0 + rows, rows * 2
    return dict(size=size, centre=ctr, cov=covs, aveCost=None, cmap=cmap)


def dist_cov(kind, D, rng):
    if kind == NULLC:
        return None
    if kind == FULLC:
        A = rng.normal(0, 1, (D, 2 * D))
        S = A @ A.T / (2 * D) + 0.5 * np.eye(D)
        return np.array([S[i, j] for i in range(D) for j in range(i + 1)], f32)
    return rng.uniform(0.5, 2.0, D).astype(f32)


# name: (tree, kind, D, N, nc, data, min_clust).  N: 3 workgroups and a ragged one (769), more than one rank chunk (1025, 3073), N = nc.
# data "dup": vectors on a coarse grid (equal distances: ties of the strict minimum); "outlier": many identical items, a small crowd
# and one far item, so that a cluster comes out below MINCLUSTSIZE and the repair fires.
CASES = {
    "flat-null-13": (False, NULLC, 13, 3073, 5, "rand", 3),
    "flat-null-1-dup": (False, NULLC, 1, 769, 64, "dup", 3),
    "flat-diag-39": (False, DIAGC, 39, 1025, 5, "rand", 3),
    "flat-invdiag-13": (False, INVDIAGC, 13, 769, 64, "rand", 3),
    "flat-full-13": (False, FULLC, 13, 769, 5, "rand", 3),
    "flat-full-39": (False, FULLC, 39, 769, 2, "rand", 3),
    "flat-repair": (False, NULLC, 2, 300, 5, "outlier", 3),
    "flat-n-eq-nc": (False, NULLC, 13, 5, 5, "rand", 1),
    "tree-null-13": (True, NULLC, 13, 3073, 8, "rand", 3),
    "tree-diag-1-dup": (True, DIAGC, 1, 769, 2, "dup", 3),
    "tree-invdiag-39": (True, INVDIAGC, 39, 769, 8, "rand", 3),
    "tree-full-13": (True, FULLC, 13, 1025, 8, "rand", 3),
    "tree-n-eq-nc": (True, NULLC, 13, 2, 2, "rand", 3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    tree, kind, D, N, nc, data, min_clust = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 7)
    if data == "dup":
        X = rng.integers(0, 400, (N, D)).astype(f32) / f32(4)
    elif data == "outlier":
        X = np.concatenate([np.tile(rng.normal(0, 1, (1, D)), (N - 21, 1)), rng.normal(3, 0.5, (20, D)), np.full((1, D), 50.0)]).astype(f32)
        X = X[rng.permutation(N)]
    else:
        X = (rng.normal(0, 3, (8, D))[rng.integers(0, 8, N)] + rng.normal(0, 1, (N, D))).astype(f32)
    cov = dist_cov(kind, D, rng)
    ref, facts = (ref_tree(X, nc, kind, cov), {}) if tree else ref_flat(X, nc, kind, cov, min_clust)
    for a in ([X] if cov is None else [X, cov]):
        a.setflags(write=False)
    return X, cov, ref, facts


def run(name):
    tree, kind, D, N, nc, _, min_clust = CASES[name]
    X, cov, ref, _ = case(name)
    dX = capi.DevArray(X)
    try:
        return capi.vq_cluster(dX.ptr, N, D, nc, tree=tree, dist_kind=kind, dist_cov=cov, min_clust_size=min_clust)
    except capi.HtkAmdError as e:
        return e.rc
    finally:
        dX.free()


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cluster_matches_the_restatement_bit_for_bit(name):
    _, _, ref, facts = case(name)
    got = run(name)
    if name == "flat-null-1-dup":
        assert facts["ties"] > 0
    if name == "flat-repair":
        assert facts["repairs"] > 0
    if isinstance(ref, int):
        assert got == ref
        return
    assert not isinstance(got, int), got
    assert np.array_equal(got["size"], ref["size"])
    assert np.array_equal(got["cmap"], ref["cmap"])
    assert same_bytes(got["centre"], ref["centre"])
    if ref["cov"] is not None:
        assert same_bytes(got["cov"], ref["cov"])
    if ref["aveCost"] is not None:
        assert same_bytes(got["aveCost"], ref["aveCost"])


@pytest.mark.parametrize("name", ["flat-invdiag-13", "tree-full-13"])
def test_two_runs_give_the_same_bytes(name):
    a, b = run(name), run(name)
    for k in ("size", "cmap", "centre", "cov", "aveCost"):
        assert same_bytes(a[k], b[k]), k


# ---- the coder
def node_scores(x, st, kind):
    """VQNodeScore (HVQ.c:414) of every frame against every node: float32 sums in the reference's order."""
    D = x.shape[1]
    df = x[:, None, :] - st["mean"][None, :, :]
    s = np.zeros(df.shape[:2], f32)
    if kind == FULLC:
        c = st["cov"]
        for i in range(1, D):
            for j in range(i):
                s += df[:, :, i] * df[:, :, j] * c[None, :, tri(i, j)]
        s *= f32(2)
        for i in range(D):
            s += df[:, :, i] * df[:, :, i] * c[None, :, tri(i, i)]
    else:
        for d in range(D):
            q = df[:, :, d] * df[:, :, d]
            s += q * st["cov"][None, :, d] if kind == INVDIAGC else q
    return st["gconst"][None, :] + s


def ref_code(X, tab):
    out, col = np.zeros((len(X), tab.num_streams), np.int16), 0
    for s in range(tab.num_streams):
        st, D = tab.stream(s), int(tab.width[s])
        sc = node_scores(X[:, col:col + D], st, tab.kind)
        col += D
        if tab.type == capi.VQ_LINTREE:
            out[:, s] = st["vqidx"][np.argmin(sc, axis=1)]
        else:
            n = np.zeros(len(X), np.int64)
            for _ in range(len(st["vqidx"])):
                r, l = st["right"][n], st["left"][n]
                nxt = np.where(sc[np.arange(len(X)), r] < sc[np.arange(len(X)), l], r, l)
                n = np.where(r >= 0, nxt, n)
            out[:, s] = st["vqidx"][n]
    return out


def random_table(tree, kind, widths, K, seed):
    rng = np.random.default_rng(seed)
    nodes = 2 * K - 1 if tree else K
    cs = []
    for D in widths:
        cov = None if kind == NULLC else np.stack([dist_cov(kind, D, rng) for _ in range(nodes)])
        cs.append(dict(size=np.ones(nodes, np.int32), centre=(rng.integers(-8, 9, (nodes, D)) / 2).astype(f32), cov=cov, tree=tree))
    return capi.VQ(clusters=cs, kind=kind, magic=9)


# K = 1; K = 320 is more than one LDS tile for every kind at these widths (a FULLC tile holds 14 nodes of 39 values)
@pytest.mark.parametrize("tree, kind, widths, K, T", [
    (False, NULLC, (39,), 320, 257), (False, INVDIAGC, (13, 13, 13), 320, 65), (False, FULLC, (39,), 40, 65), (False, FULLC, (5, 4, 3), 1, 1),
    (False, INVDIAGC, (7,), 1, 257), (True, NULLC, (13, 13, 13), 8, 257), (True, INVDIAGC, (39,), 64, 65), (True, FULLC, (13,), 16, 257),
    (True, FULLC, (3, 2, 1), 1, 1), (True, NULLC, (1,), 2, 65)])
def test_codes_match_the_restatement(tree, kind, widths, K, T):
    tab = random_table(tree, kind, widths, K, seed=K + T)
    rng = np.random.default_rng(T)
    X = (rng.integers(-16, 17, (T, sum(widths))) / 4).astype(f32)      # a coarse grid: equal scores occur
    dX = capi.DevArray(X)
    got = tab.code(dX.ptr, [0, T // 2, T], sum(widths))
    dX.free()
    assert np.array_equal(got, ref_code(X, tab))


@pytest.mark.parametrize("name", ["lin", "tree"])
def test_codes_match_the_reference_hcopy_file(name, tmp_path):
    """tests/golden/vq/<name>_a.dis: what the reference's HCopy wrote for a.mfc with VQTABLE = <name>.vq (make_vq_golden.py)."""
    X, _, _ = capi.parm_read(os.path.join(GOLD, "a.mfc"))[:3]
    tab = capi.VQ(path=os.path.join(GOLD, name + ".vq"))
    dX = capi.DevArray(X)
    codes = tab.code(dX.ptr, [0, len(X)], X.shape[1])
    dX.free()
    capi.parm_write_discrete(str(tmp_path / "a.dis"), codes, 100000, withCrc=True)
    assert open(tmp_path / "a.dis", "rb").read() == open(os.path.join(GOLD, name + "_a.dis"), "rb").read()


@pytest.mark.parametrize("name, tree, kind, nc, glob", [("lin", False, INVDIAGC, (6,), False), ("lin_g", False, INVDIAGC, (6,), True), ("tree", True, FULLC, (4, 2), False)])
def test_hquant_golden_table_from_the_device(name, tree, kind, nc, glob, tmp_path):
    """HQuant end to end: the pools of a.mfc + b.mfc clustered on the device, the table written: the reference's bytes."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "..", "examples"))
    import hquant_codebook
    out = str(tmp_path / "t.vq")
    hquant_codebook.main((["-f"] if kind == FULLC else ["-d"]) + (["-g"] if glob else []) + (["-t"] if tree else []) + ["-s", str(len(nc))] +
                         [a for s, k in enumerate(nc) for a in ("-n", str(s + 1), str(k))] + [out, os.path.join(GOLD, "a.mfc"), os.path.join(GOLD, "b.mfc")])
    assert open(out, "rb").read() == open(os.path.join(GOLD, name + ".vq"), "rb").read()
