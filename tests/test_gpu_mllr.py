"""MLLR mean transforms on the device (csrc/mllr.hip): the class statistics, the sums up the tree, the solves, apply / restore -- from
planted tables through capi.mllr_probe against numpy fp64, and the committed task against the reference's HERest -u a.

The numpy side restates AccMLLRPDFStats: icov = 1 / var, scale = occ * icov, (scale * xi_j) * xi_k and (spSum * xi_j) * icov as float32
products (a factor 1.0 for the bias entry is exact), summed in fp64.  The solve is numpy.linalg.solve on the symmetric matrix."""
import json
import os

import numpy as np
import pytest

from htk_amd import capi

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TREE3 = [(2, 3), (0, 0), (4, 5), (0, 0), (0, 0)]          # three classes: nodes 2, 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mllr")
ERANGE = -7


def class_terms(mean, var, occ, sp, members, c0, bs):
    """Per member and row of the block the fp64 values of the float32 terms: G [n, bs, d, d] (lower triangle meaningful), k [n, bs, d]."""
    n = len(members)
    xi = np.concatenate([mean[members, c0:c0 + bs], np.ones((n, 1), f32)], axis=1).astype(f32)
    icov = (f32(1.0) / var[members, c0:c0 + bs]).astype(f32)
    scale = (occ[members, None].astype(f32) * icov).astype(f32)
    G = ((scale[:, :, None, None] * xi[:, None, :, None]).astype(f32) * xi[:, None, None, :]).astype(f32)
    k = ((sp[members, c0:c0 + bs, None].astype(f32) * xi[:, None, :]).astype(f32) * icov[:, :, None]).astype(f32)
    return G.astype(f64), k.astype(f64)


def node_members(children, cls):
    """Members (in the set's order per class, classes in node order) of every node, as the reference's AccNodeStats visits them."""
    term = [i for i, k in enumerate(children) if k == (0, 0)]
    mem = {}

    def walk(i):
        if children[i] == (0, 0):
            mem[i] = np.nonzero(cls == term.index(i) + 1)[0]
        else:
            mem[i] = np.concatenate([walk(children[i][0] - 1), walk(children[i][1] - 1)])
        return mem[i]
    walk(0)
    return [mem[i] for i in range(len(children))]


def np_records(mean, var, occ, sp, cls, children, blocks, min_occ=0.0, reverse=False):
    """The records of capi.mllr_probe's statistics in numpy: sequential fp64 sums in member order, or in the opposite order."""
    D = mean.shape[1]
    rows, rec = capi.mllr_record_offsets(D, blocks)
    out = np.zeros((len(children), rec))
    add = lambda a: np.cumsum(a[::-1] if reverse else a, axis=0)[-1] if len(a) else a.sum(axis=0)
    for node, members in enumerate(node_members(children, cls)):
        out[node, rec - 1] = add(occ[members].astype(f32).astype(f64)) if len(members) else 0.0
        use = members[occ[members].astype(f32) > f32(min_occ)]
        c0 = 0
        for bs in blocks:
            d = bs + 1
            G, k = class_terms(mean, var, occ, sp, use, c0, bs)
            Gs, ks = add(G), add(k)
            tri = np.tril_indices(d)
            for i in range(bs):
                off = rows[c0 + i][0]
                out[node, off:off + d * (d + 1) // 2] = Gs[i][tri]
                out[node, off + d * (d + 1) // 2:off + d * (d + 1) // 2 + d] = ks[i]
            c0 += bs
    return out


def np_solve(record, D, blocks, use_bias):
    """fp64 rows W [D, maxd] from one node's record."""
    rows, _ = capi.mllr_record_offsets(D, blocks)
    W = np.zeros((D, max(blocks) + 1))
    for i, (off, c0, bs) in enumerate(rows):
        d = bs + 1
        n = d if use_bias else bs
        L = np.zeros((d, d))
        L[np.tril_indices(d)] = record[off:off + d * (d + 1) // 2]
        Gm = L + np.tril(L, -1).T
        W[i, :n] = np.linalg.solve(Gm[:n, :n], record[off + d * (d + 1) // 2:off + d * (d + 1) // 2 + n])
    return W


def plant(D, blocks, sizes, seed, use_bias=True):
    """Three classes of the given sizes with distinct random means and spSum = occ (A mu + b) in fp64, A block diagonal and well conditioned."""
    rng = np.random.RandomState(seed)
    G = sum(sizes)
    mean = (rng.randn(G, D) * 2.0).astype(f32)
    var = (0.5 + rng.rand(G, D)).astype(f32)
    occ = 1.0 + 9.0 * rng.rand(G)
    cls = np.repeat(np.arange(1, len(sizes) + 1), sizes).astype(np.int32)
    perm = rng.permutation(G)                              # classes interleaved in the set's order
    cls = cls[perm]
    A = np.zeros((len(sizes), D, D)); b = np.zeros((len(sizes), D))
    for c in range(len(sizes)):
        o = 0
        for bs in blocks:
            A[c, o:o + bs, o:o + bs] = np.eye(bs) + 0.3 * rng.randn(bs, bs) / np.sqrt(bs)
            o += bs
        if use_bias:
            b[c] = rng.randn(D)
    sp = occ[:, None] * (np.einsum("gij,gj->gi", A[cls - 1], mean.astype(f64)) + b[cls - 1])
    return mean, var, occ, sp, cls, A, b


def ulp32(x):
    return np.spacing(np.abs(x).astype(f32)).astype(f64)


def check_rows(out, Wnp, D, blocks, use_bias, k):
    """Transform k of the probe against numpy's fp64 rows: the float output is numpy's row rounded to float; where the two fp64 solves differ
    (by less than one float ulp -- more is an error) the rounded values may differ by one ulp.  Returns the largest deviation in float ulps."""
    rows, _ = capi.mllr_record_offsets(D, blocks)
    worst = 0.0
    for i, (off, c0, bs) in enumerate(rows):
        n = bs + 1 if use_bias else bs
        wd, wn = out["W"][k, i, :n], Wnp[i, :n]
        got = np.concatenate([out["A"][k, i, c0:c0 + bs], out["bias"][k, i:i + 1] if use_bias else []]).astype(f32)
        assert np.array_equal(got, wd.astype(f32)), "the float row is not the fp64 row rounded"
        u = ulp32(wn)
        assert (np.abs(wd - wn) < u).all(), (i, np.abs(wd - wn).max(), u.min())
        same = wd == wn
        assert np.array_equal(got[same], wn.astype(f32)[same])
        assert (np.abs(got.astype(f64) - wn.astype(f32).astype(f64)) <= u).all()
        worst = max(worst, float((np.abs(got.astype(f64) - wn.astype(f32).astype(f64)) / u).max()))
        assert not out["A"][k, i, :c0].any() and not out["A"][k, i, c0 + bs:].any()
    return worst


def sizes_for(D, blocks, which):
    d = max(blocks) + 1
    small = [(d + 1, 31, 33), (63, 64, 65)] if d + 1 <= 31 else [(d + 1, 64, 65), (63, 96, 97)]
    return small[which]


CASES = [(D, blocks, bias, which) for D in (1, 5, 39, 45) for blocks in ([D], [13, 13, 13], [1, D - 1]) for bias in (True, False) for which in (0, 1)
         if sum(blocks) == D and min(blocks) >= 1 and not (D == 1 and blocks != [1])]


@pytest.mark.parametrize("D, blocks, bias, which", CASES)
def test_recovery_of_a_planted_transform(D, blocks, bias, which):
    """spSum = occ (A mu + b).  G, k and the occupation of every class equal the numpy restatement from the planted tables bit for bit (a
    terminal's fp64 sums run in the same order), the inner nodes' within one fp64 ulp of the entry per addition; the estimate is numpy's
    fp64 solve of the RESTATEMENT's statistics rounded to float (check_rows) -- nothing of the device enters the reference -- and it is the planted
    transform within the error that rounding spSum to float and the float factors put into a row: 8 * 2^-24 * cond(G_i) * max|w| -- the class
    sizes run from one over the smallest solvable (block + 2) across the chunk of 32 (31, 33), the wavefront (63, 64, 65) and three chunks."""
    sizes = sizes_for(D, blocks, which)
    mean, var, occ, sp, cls, A, b = plant(D, blocks, sizes, seed=100 + D + len(blocks) + which, use_bias=bias)
    out = capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e-3, use_bias=bias, blocks=blocks)
    assert out["status"] == 0 and out["x_node"] == [2, 4, 5] and out["class_xform"] == [1, 2, 3]
    ref = np_records(mean, var, occ, sp, cls, TREE3, blocks)
    rows, _ = capi.mllr_record_offsets(D, blocks)
    assert np.array_equal(out["node_occ"][[1, 3, 4]], ref[[1, 3, 4], -1])
    for node in (0, 2):                                                  # inner nodes: children's sums added, another fp64 order than the restatement's
        assert (np.abs(out["stats"][node] - ref[node]) <= 2.0 * np.spacing(np.abs(ref[node])) + 2.0 ** -52 * np.abs(ref[node]).max()).all()
    for k, node in enumerate(out["x_node"]):
        assert np.array_equal(out["stats"][node - 1], ref[node - 1]), "the class's statistics are not the restatement's"
        Wnp = np_solve(ref[node - 1], D, blocks, bias)                  # numpy alone, from the planted tables
        worst = check_rows(out, Wnp, D, blocks, bias, k)
        print("D %d blocks %s bias %s sizes %s class %d: largest deviation %.2f float ulp" % (D, blocks, bias, sizes, k + 1, worst))
        for i, (off, c0, bs) in enumerate(rows):
            d = bs + 1
            n = d if bias else bs
            L = np.zeros((d, d)); L[np.tril_indices(d)] = ref[node - 1, off:off + d * (d + 1) // 2]
            cond = np.linalg.cond((L + np.tril(L, -1).T)[:n, :n])
            true = np.concatenate([A[k, i, c0:c0 + bs], b[k, i:i + 1] if bias else []])
            tol = 8.0 * 2.0 ** -24 * cond * np.abs(true).max()
            assert np.abs(Wnp[i, :n] - true).max() <= tol, (i, cond)
            assert np.abs(out["W"][k, i, :n] - true).max() <= tol, (i, cond)


@pytest.mark.parametrize("D, blocks", [(5, [2, 3]), (39, [39]), (39, [13, 13, 13])])
def test_statistics_of_every_node(D, blocks):
    """G, k and the occupation of every node, terminals and inner, against the restatement with sequential fp64 sums in the reference's member
    order.  The bound is relative to the node's largest entry: 4 x the largest spread, over the nodes, between that restatement and the same
    terms summed in the opposite order -- what fp64 reordering alone does.  The terms are float values, so most fp64 sums of a few hundred of
    them are exact; measured: spread 8.5e-17 (D 5) and 2.1e-16 (D 39), so the bounds are 3.4e-16 and 8.5e-16.  Two runs are bit-equal."""
    sizes = (200, 333, 257)
    mean, var, occ, sp, cls, _, _ = plant(D, blocks, sizes, seed=7 + D)
    out = capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e-3, blocks=blocks)
    again = capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e-3, blocks=blocks)
    assert np.array_equal(out["stats"], again["stats"]) and np.array_equal(out["A"], again["A"]) and np.array_equal(out["bias"], again["bias"])
    seq = np_records(mean, var, occ, sp, cls, TREE3, blocks)
    pair = np_records(mean, var, occ, sp, cls, TREE3, blocks, reverse=True)
    scale = np.abs(seq[:, :-1]).max(axis=1)
    spread = float((np.abs(seq - pair)[:, :-1].max(axis=1) / scale).max())
    print("D %d blocks %s: spread %.3g" % (D, blocks, spread))
    assert spread > 0.0
    for node in range(len(TREE3)):
        dev = np.abs(out["stats"][node, :-1] - seq[node, :-1]).max() / scale[node]
        print("   node %d: device %.3g" % (node + 1, dev))
        assert dev <= 4.0 * spread
        assert abs(out["node_occ"][node] - seq[node, -1]) <= 4.0 * spread * seq[node, -1]
    assert np.array_equal(out["stats"][[1, 3, 4]], seq[[1, 3, 4]])      # a terminal's sums are in the same order: the same bits


def test_min_occ_thresh_leaves_gaussians_out():
    """Gaussians at and below MINOCCTHRESH enter no sum of G and k; the node occupation (SetNodeOcc) counts them all the same."""
    D, blocks = 5, [5]
    mean, var, occ, sp, cls, _, _ = plant(D, blocks, (40, 50, 60), seed=3)
    occ[::3] = 2.0
    occ[1::7] = 1.5
    out = capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e-3, blocks=blocks, min_occ_thresh=2.0)
    keep = occ > 2.0
    assert 0 < keep.sum() < len(occ)
    cls2 = np.where(keep, cls, 0).astype(np.int32)
    ref = np_records(mean, var, occ, sp, cls2, TREE3, blocks)
    assert np.array_equal(out["stats"][[1, 3, 4], :-1], ref[[1, 3, 4], :-1])
    full = np_records(mean, var, occ, sp, cls, TREE3, blocks)
    assert np.array_equal(out["node_occ"][[1, 3, 4]], full[[1, 3, 4], -1])
    assert not np.array_equal(full[1, :-1], ref[1, :-1])


def test_root_below_the_threshold_gives_no_set():
    mean, var, occ, sp, cls, _, _ = plant(5, [5], (20, 20, 20), seed=5)
    out = capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e9, blocks=[5])
    assert out["status"] == capi.MLLR_NOSET and out["x_node"] == [] and out["class_xform"] == [0, 0, 0]


def test_a_singular_class_is_refused_with_its_node():
    """Class 2 (node 4) has 3 distinct means for a block of 5 with bias (6 unknowns a row): HTKAMD_ERANGE, naming the node."""
    D, blocks = 5, [5]
    mean, var, occ, sp, cls, _, _ = plant(D, blocks, (30, 30, 30), seed=9)
    idx = np.nonzero(cls == 2)[0]
    mean[idx] = mean[idx[:3]][np.arange(len(idx)) % 3]
    with pytest.raises(capi.HtkAmdError) as e:
        capi.mllr_probe(mean, var, occ, sp, cls, TREE3, split_thresh=1e-3, blocks=blocks)
    assert e.value.rc == ERANGE and e.value.bad_node == 4 and "node 4, row" in str(e.value) and "nothing is installed" in str(e.value)


# ------------------------------------------------------------------------------------------ apply and restore
def np_apply(mean, A, b, gauss_x, blocks):
    """mean' = A mean + b as the kernel states it: float32 products, float32 sums in index order, the bias last."""
    out = mean.copy()
    for g in range(len(mean)):
        x = gauss_x[g]
        if x < 0:
            continue
        c0 = 0
        for bs in blocks:
            for i in range(c0, c0 + bs):
                v = f32(A[x, i, c0]) * mean[g, c0]
                for j in range(c0 + 1, c0 + bs):
                    v = f32(v + f32(A[x, i, j]) * mean[g, j])
                out[g, i] = f32(v + b[x, i])
            c0 += bs
    return out


def test_apply_and_restore():
    """Three classes and some Gaussians in none.  The means after apply are np_apply's bit for bit; htkamd_outp_block's scores are those of a
    model made from the adapted means (the derived tables were rebuilt); after restore means and scores are the first ones, bit for bit."""
    from htk_amd import synth
    s = synth.generate(NS=12, M=3, NP=6, NU=2, T=40, seed=5)
    pk = s.packed()
    model = capi.Model(pk)
    G, D = model.G, model.D
    blocks = [D] if D % 3 else [D // 3] * 3
    rng = np.random.RandomState(2)
    A = np.zeros((3, D, D), f32)
    for x in range(3):
        o = 0
        for bs in blocks:
            A[x, o:o + bs, o:o + bs] = (np.eye(bs) + 0.1 * rng.randn(bs, bs)).astype(f32)
            o += bs
    b = rng.randn(3, D).astype(f32)
    cls = (np.arange(G) % 4).astype(np.int32)                          # 0: in no class
    xs = capi.Mllr.from_tables(A, b, [2, 3, 1], blocks=blocks)
    X = np.concatenate(s.feats)[:50]
    states = np.arange(model.S, dtype=np.int32)
    before = model.outp_block(X, states)
    mean0 = model.get_params()["mean"].copy()
    xs.apply(model, cls)
    want = np_apply(mean0, A, b, np.array([-1, 1, 2, 0])[cls], blocks)
    got = model.get_params()["mean"]
    assert np.array_equal(got, want) and not np.array_equal(got, mean0) and np.array_equal(got[cls == 0], mean0[cls == 0])
    pk2 = dict(pk)
    pk2["mean"] = want
    assert np.array_equal(model.outp_block(X, states), capi.Model(pk2).outp_block(X, states))
    for mode in (capi.SCORE_BF16,):
        assert np.array_equal(model.outp_block(X, states, mode), capi.Model(pk2).outp_block(X, states, mode))
    with pytest.raises(capi.HtkAmdError) as e:
        xs.apply(model, cls)
    assert "adapted already" in str(e.value) and "parent transform" in str(e.value)
    capi.Mllr.restore(model)
    assert np.array_equal(model.get_params()["mean"], mean0) and np.array_equal(model.outp_block(X, states), before)
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.restore(model)
    assert "not adapted" in str(e.value)


# ------------------------------------------------------------------------------------------ against the reference
def fixture_pass():
    import regtree_util as ru
    mmf = capi.Mmf([os.path.join(GOLDEN, "hmmdefs")], hmm_list=os.path.join(GOLDEN, "hmmlist"))
    model = capi.Model(mmf.packed())
    mlf = capi.Mlf(os.path.join(GOLDEN, "labels.mlf"))
    files = [l.strip() for l in open(os.path.join(GOLDEN, "train.scp")) if l.strip()]
    feats = [capi.parm_read(os.path.join(GOLDEN, f))[0] for f in files]
    seqs = [np.array([mmf.logical[n] for n, _, _, _ in mlf.find(os.path.splitext(f)[0] + ".lab")], np.int32) for f in files]
    batch = capi._Batch(feats, np.float32)
    fb, acc = capi.ForwardBackward(model), capi.Accs(model)
    fb.prepare(batch.dev.ptr.value, batch.off, capi.offsets([len(q) for q in seqs]), np.concatenate(seqs))
    fb.execute(capi.fb_config(), acc)
    assert (fb.results()[1] == 1).all()
    kids = ru.parse_tree(open(os.path.join(GOLDEN, "rtree.tree")).read())
    classes = ru.parse_base(open(os.path.join(GOLDEN, "rtree.base")).read())
    tree = capi.RegTree.from_tables(kids, dict(zip([i + 1 for i, k in enumerate(kids) if k == (0, 0)], classes)))
    return mmf, model, acc, tree, (batch, fb)


def test_against_the_reference_transform_file(tmp_path):
    """The committed task (tests/golden/mllr): one exact-mode pass, then the estimate at the `one` threshold, where the smallest terminal's
    class takes its parent's transform.  Number of transforms, class map, node set and node occupations as the reference's; every entry of
    A and b within the bound kept in the fixture: 4 x the largest difference between the reference's results for two orders of the files
    (1.68e-06, so 6.7e-06), at least one float ulp of the entry.  The reference sums its statistics in float over the frames; that noise belongs
    to a row, so one figure serves every entry.  Then a singular request on the same model: HTKAMD_ERANGE, nothing installed, the scores
    unchanged bit for bit; then the estimated set applied and restored."""
    ref = json.load(open(os.path.join(GOLDEN, "ref.json")))
    case = ref["cases"]["one"]
    mmf, model, acc, tree, keep = fixture_pass()
    xs = capi.Mllr.estimate(mmf, model, acc, tree, split_thresh=case["thresh"], blocks=ref["blocks"])
    want = capi.Mllr.read(os.path.join(GOLDEN, "xf_one", "sp1.mllr"))
    assert xs.status == 0 and xs.num_xforms == want.num_xforms == case["numXforms"] and xs.class_xform == want.class_xform
    small = ref["fallback"]["terminal"]
    parent = next(i + 1 for i, k in enumerate(ref["children"]) if small in k)
    assert xs.xform_nodes == [parent if n == small else n for n in (4, 5, 6, 7)]
    occ = xs.node_occ()
    for n, o in case["nodeOcc"].items():
        assert abs(occ[int(n) - 1] - o) <= 1e-4 * o, (n, occ[int(n) - 1], o)      # (the trace prints floats summed in float)
    worst, over, total = 0.0, [], 0
    for k in range(1, want.num_xforms + 1):
        (A, b), (Ar, br) = xs.xform(k), want.xform(k)
        parts, c0 = [("bias", b.astype(f64), br)], 0
        for bs in ref["blocks"]:
            parts.append(("block at %d" % c0, A[c0:c0 + bs, c0:c0 + bs].astype(f64), Ar[c0:c0 + bs, c0:c0 + bs].astype(f64)))
            c0 += bs
        parts = [(what, np.abs(got - val), np.maximum(ref["bound"], ulp32(val)), val) for what, got, val in parts]
        for what, dev, bnd, val in parts:
            total += dev.size
            worst = max(worst, float((dev / bnd).max()))
            for idx in zip(*np.nonzero(dev > bnd)):
                over.append("transform %d %s %s: value %.7e, deviation %.3g, bound %.3g" % (k, what, idx, val[idx], dev[idx], bnd[idx]))
    print("largest deviation from the reference: %.3f of the bound; %d of %d entries over it" % (worst, len(over), total))
    print("\n".join(over))
    xs.set_names("sp1.mllr")
    xs.write(tmp_path / "sp1.mllr")
    again = capi.Mllr.read(tmp_path / "sp1.mllr")
    assert again.class_xform == xs.class_xform and np.allclose(again.xform(2)[0], xs.xform(2)[0], rtol=1e-6, atol=0.0)      # (%e: 7 significant digits)
    # a singular request: blocks of 6 with bias need 7 distinct means a class; min_occ_thresh leaves too few in
    X = np.concatenate([capi.parm_read(os.path.join(GOLDEN, "data", "sp1_f00.usr"))[0]])
    states = np.arange(model.S, dtype=np.int32)
    before = model.outp_block(X, states)
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.estimate(mmf, model, acc, tree, split_thresh=1e-3, blocks=[6], min_occ_thresh=float(np.sort(acc.download()["muOcc"])[-8]))
    assert e.value.rc == ERANGE and "node" in str(e.value) and "row" in str(e.value)
    assert np.array_equal(model.outp_block(X, states), before)
    # and the estimated set applied: the aligner's scorer runs on the adapted means
    xs.apply(model)
    assert not np.array_equal(model.outp_block(X, states), before)
    capi.Mllr.restore(model)
    assert np.array_equal(model.outp_block(X, states), before)
    assert not over, over
