"""Data-driven state clustering on the device (htk_amd/csrc/datacluster.hip + htk_amd/host/treeclust.c): the item distances bit for bit
against numpy restatements that round where the reference rounds, the merge logs against a literal restatement of Clustering +
RemOutliers (tests/datacluster_util.py), the tied sets byte for byte against the reference's HHEd (tests/golden/datacluster)."""
import importlib.util
import os
import re

import numpy as np
import pytest

import datacluster_util as du
import treeclust_util as tu

pytestmark = pytest.mark.gpu

HHED = os.path.join(tu.ROOT, "oracle", "_ref", "HHEd")


def write_set(path, lst, mean, var, weights=None):
    """One three-state model per row of mean / var ([N][M][V]; weights [N][M], a row's zero weights end its mixture)."""
    N, V = mean.shape[0], mean.shape[-1]
    with open(path, "w") as f:
        f.write("~o <STREAMINFO> 1 %d <VECSIZE> %d <NULLD><USER><DIAGC>\n" % (V, V))
        for i in range(N):
            f.write('~h "m%d"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n' % i)
            w = None if weights is None else [x for x in weights[i] if x > 0]
            if w is not None and len(w) > 1:
                f.write("<NUMMIXES> %d\n" % len(w))
            for m in range(1 if w is None else len(w)):
                if w is not None and len(w) > 1:
                    f.write("<MIXTURE> %d %s\n" % (m + 1, repr(float(w[m]))))
                f.write("<MEAN> %d\n %s\n<VARIANCE> %d\n %s\n" % (V, " ".join(repr(float(x)) for x in mean[i, m]), V, " ".join(repr(float(x)) for x in var[i, m])))
            f.write("<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n")
    with open(lst, "w") as f:
        f.write("\n".join("m%d" % i for i in range(N)) + "\n")


def items_in_order(m):
    il = m.item_list("{*.state[2]}")
    pk = m.packed()
    st = [int(pk["hmmState"][pk["hmmStateOff"][h]]) for h, _ in il]
    return pk, st


@pytest.mark.parametrize("V", [1, 5, 39])
def test_divergence_distances_are_bit_equal(native, tmp_path, V):
    rng = np.random.RandomState(V)
    for N in (1, 2, 63, 64, 65, 130):
        mean = (rng.randn(N, 1, V) * 3).astype(np.float32)
        var = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (N, 1, V))).astype(np.float32)      # six decades
        if N > 2:
            mean[N - 1] = mean[1]; var[N - 1] = var[1]                                          # two identical states
        write_set(tmp_path / "set", tmp_path / "lst", mean, var)
        m = native.Mmf([str(tmp_path / "set")], hmm_list=str(tmp_path / "lst"))
        pk, st = items_in_order(m)
        g = [int(pk["compGauss"][pk["stateCompOff"][s]]) for s in st]
        want = du.divergence_matrix(pk["mean"][g], pk["var"][g])
        got = native.state_distances(m, "{*.state[2]}")
        assert got.shape == (N, N)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, N, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
        if N > 2:
            assert (got == 0).sum() == N + 2


@pytest.mark.parametrize("M", [2, 3])
def test_gdistance_is_the_sum_over_the_exact_scores(native, tmp_path, M):
    rng = np.random.RandomState(10 + M)
    N, V = 21, 5
    mean = (rng.randn(N, M, V) * 2).astype(np.float32)
    var = np.exp(rng.uniform(np.log(0.05), np.log(5.0), (N, M, V))).astype(np.float32)
    w = rng.uniform(0.2, 1.0, (N, M))
    w[::3, M - 1] = 0.0                                                                         # uneven mixtures
    w /= w.sum(1, keepdims=True)
    w[1] = np.array([1.0 - 5e-6] + [5e-6 / (M - 1)] * (M - 1))                                  # weights below MINMIX
    write_set(tmp_path / "set", tmp_path / "lst", mean, var, w)
    m = native.Mmf([str(tmp_path / "set")], hmm_list=str(tmp_path / "lst"))
    pk, st = items_in_order(m)
    got = native.state_distances(m, "{*.state[2]}")
    pk = m.packed()                                                                             # (the gConsts are the set's now)
    obs, off = [], [0]
    for s in st:
        for c in range(pk["stateCompOff"][s], pk["stateCompOff"][s + 1]):
            obs.append(pk["mean"][pk["compGauss"][c]])
        off.append(len(obs))
    assert len(set(np.diff(off).tolist())) > 1
    scores = native.Model(pk).outp_block(np.array(obs, np.float32), np.array(st, np.int32), mode=native.SCORE_SOUTP | native.SCORE_DIAGC)
    want = du.gdistance_matrix(scores, off)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]


def matrices(N, rng):
    def sym(a):
        a = np.triu(a, 1)
        return (a + a.T).astype(np.float32)
    return {"equal": sym(np.full((N, N), 2.5)), "integers": sym(rng.randint(1, 5, (N, N)).astype(float)), "random": sym(rng.rand(N, N) * 10 + 0.01)}


@pytest.mark.parametrize("N", [2, 3, 64, 65, 130])
def test_merge_logs_equal_the_literal_restatement(native, N):
    rng = np.random.RandomState(N)
    occ = (rng.rand(N) * 50 + 1).astype(np.float32)
    for name, d in matrices(N, rng).items():
        mx, mid = float(d.max()), float(np.median(d[np.triu_indices(N, 1)]))
        stops = [(1, 1.0e15), (N, 1.0e15), (max(N - 1, 1), 1.0e15), (1, 0.0), (1, mid), (1, mx + 1.0)]
        outliers = [None, float(np.median(occ)) * 2, 1.0e9]
        cases = [(s, o) for s in stops for o in outliers] if N <= 65 else [(stops[0], None), (stops[4], outliers[1]), (stops[3], outliers[2]), (stops[2], outliers[1])]
        for (num_req, thr), out in cases:
            want, _, _ = du.ref_clustering(d, num_req, thr, occ if out is not None else None, out or 0.0)
            got = native.cluster_merges(d, num_req, thr, occ if out is not None else None, out or 0.0)
            assert [tuple(x) for x in got.tolist()] == want, (name, N, num_req, thr, out, got[:6].tolist(), want[:6])


def test_negative_distances_are_lifted_to_zero_by_the_first_merge(native):
    rng = np.random.RandomState(3)
    d = matrices(12, rng)["random"] - 5.0
    np.fill_diagonal(d, 0.0)
    for thr in (-1.0, 0.0, 2.0):
        want, _, _ = du.ref_clustering(d, 1, thr)
        assert [tuple(x) for x in native.cluster_merges(d, 1, thr).tolist()] == want


def load(native, workdir, name=None):
    if name is None:
        mmf, lst = tu.unpack_inputs(workdir)
        return native.Mmf([mmf], hmm_list=lst)
    text = du.golden_bytes(name)
    p, lst = os.path.join(str(workdir), name), os.path.join(str(workdir), "sublist")
    open(p, "wb").write(text)
    open(lst, "w").write("\n".join(re.findall(r'^~h "([^"]+)"', text.decode(), flags=re.M)) + "\n")
    return native.Mmf([p], hmm_list=lst)


def run(native, m, script_text, workdir, stats=None):
    from htk_amd import treeclust
    sc = treeclust.parse_script(script_text)
    res = treeclust.run_script(m, sc, stats_path=stats, base_dir=str(workdir))
    out = os.path.join(str(workdir), "tied.mmf")
    m.write(m.packed(), one_file=out)
    return open(out, "rb").read(), sc, res


def first_difference(got: bytes, want: bytes, sc, counts) -> str:
    """The first command whose cluster count or membership is not HHEd's."""
    def members(text, root):
        macros = sorted(set(re.findall(r'~s "(%s\d+)"' % re.escape(root), text)), key=lambda x: int(x[len(root):]))
        return [sorted(h for h, body in re.findall(r'~h "([^"]+)"(.*?)<ENDHMM>', text, flags=re.S) if '~s "%s"' % mac in body) for mac in macros]
    g, w = got.decode(), want.decode()
    for c in [c for c in sc.commands if c[0] in ("TC", "NC")]:
        a, b = members(g, c[2]), members(w, c[2])
        if len(a) != len(b):
            return "%s %s: %d clusters, HHEd made %d" % (c[0], c[2], len(a), len(b))
        for k, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return "%s %s: cluster %d holds %s, HHEd's holds %s" % (c[0], c[2], k + 1, x, y)
    return "same clusters; the files part elsewhere"


@pytest.mark.parametrize("which", ["a", "b", "c", "e"])
def test_scripts_give_hhed_s_tied_set_byte_for_byte(native, tmp_path, which):
    m = load(native, tmp_path, "sub_mu2.mmf" if which == "e" else None)
    got, sc, res = run(native, m, open(os.path.join(du.G, which + ".hed")).read(), tmp_path, stats=os.path.join(tu.G, "stats") if which == "b" else None)
    want = du.golden_bytes("tied_%s.mmf" % which)
    assert got == want, first_difference(got, want, sc, res)


def test_live_against_hhed_with_other_thresholds(native, tmp_path):
    if not os.path.exists(HHED):
        pytest.skip("oracle/_ref/HHEd is not built")
    spec = importlib.util.spec_from_file_location("make_datacluster_golden", os.path.join(tu.ROOT, "tests", "golden", "make_datacluster_golden.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    for ro in (25.0, 120.0):
        ref = tmp_path / ("ref%d" % ro); ref.mkdir()
        tu.unpack_inputs(ref)
        (ref / "stats").write_bytes(open(os.path.join(tu.G, "stats"), "rb").read())
        (ref / "s.hed").write_text(gen.script("b", ro))
        gen.run_hhed(str(ref), "hmmdefs", "hmmlist", "s.hed", "tied.mmf")
        mine = tmp_path / ("mine%d" % ro); mine.mkdir()
        got, sc, res = run(native, load(native, mine), gen.script("b", ro), mine, stats=os.path.join(tu.G, "stats"))
        want = (ref / "tied.mmf").read_bytes()
        assert got == want, (ro, first_difference(got, want, sc, res))


def test_tb_and_tc_in_one_script_equal_the_parts_in_turn(native, tmp_path):
    tree = open(os.path.join(tu.G, "script1.hed")).read().splitlines()
    head = [ln for ln in tree if ln[:2] in ("RO", "QS")]
    tb = [ln for ln in tree if ln.startswith("TB") and '"*-a+*"' in ln]
    tc = [ln for ln in open(os.path.join(du.G, "a.hed")).read().splitlines() if '"*-a+*"' not in ln]
    assert len(tb) == 3 and len(tc) == 24
    stats = os.path.join(tu.G, "stats")
    (tmp_path / "one").mkdir(); (tmp_path / "two").mkdir()
    one, _, _ = run(native, load(native, tmp_path / "one"), "\n".join(head + tb + tc) + "\n", tmp_path / "one", stats=stats)
    m = load(native, tmp_path / "two")
    run(native, m, "\n".join(head + tb) + "\n", tmp_path / "two", stats=stats)
    two, _, _ = run(native, m, "\n".join(head[:1] + tc) + "\n", tmp_path / "two", stats=stats)
    assert one == two
    assert b'~s "ST_a_2_' in one and b'~s "TC_b_2_1"' in one
