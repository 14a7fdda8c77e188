"""Lattice rescoring on the device (htkamd_latset_best / _fb_max / _prune) against the reference's recorded files and, where no fixture
exists, against the restatement in latrescore_util.py (which test_latrescore_host.py pins to the reference on the CPU).  Nothing here has a
tolerance: paths, totals, Fw, Bw, best and the keep flags compare with array_equal, files byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import latrescore_util as lu
import make_latrescore_golden as gen

pytestmark = pytest.mark.gpu
ROOT = lu.ROOT
RUNS = lu.fixtures()["runs"]
F5 = ["f_default", "f_s5_pm10", "f_s0_p3_a05", "f_s12_pm2_r25_a15", "f_s2_r0"]


@pytest.fixture(scope="module")
def groups(native, tmp_path_factory):
    out = {}
    for g in lu.fixtures()["groups"]:
        d = str(tmp_path_factory.mktemp("lat_" + g))
        dpath, lats = lu.unpack_group(g, d)
        out[g] = dict(dir=d, dict_path=dpath, paths=lats, names=sorted(lats))
    return out


@pytest.fixture(scope="module")
def pool(native, groups):
    """Every fixture lattice by name, as the restatement reads it, with its orders (computed once)."""
    p = {}
    for g, G in groups.items():
        if g in ("random", "big", "rescore"):
            for n in G["names"]:
                l = lu.read_slf(G["paths"][n])
                p[(g if g == "rescore" else "") + n] = dict(path=G["paths"][n], lat=l, orders=lu.orders(l), dict_path=G["dict_path"])
    return p


def settings_for(K):
    rng = np.random.RandomState(7 + K)
    base = [lu.setting_of(r["args"]) for r in RUNS if r["group"] == "random" and r["name"] in F5]
    more = [(round(rng.uniform(0.3, 2), 2), round(rng.uniform(0, 20), 1), round(rng.uniform(-20, 5), 2), round(rng.uniform(0, 3), 1)) for _ in range(max(K - 5, 0))]
    return (base + more)[:K]


@pytest.mark.parametrize("rid", [r["id"] for r in RUNS])
def test_the_tool_writes_the_references_files(native, groups, rid, tmp_path, monkeypatch):
    """examples/hlrescore_batch.py with the run's switches: .rec, MLF and .lat byte for byte."""
    import hlrescore_batch
    run = next(r for r in RUNS if r["id"] == rid)
    G = groups[run["group"]]
    os.makedirs(str(tmp_path / "in")); os.makedirs(str(tmp_path / "out"))
    for n in run["lats"]:
        os.symlink(G["paths"][n], str(tmp_path / "in" / (n + ".lat")))
    (tmp_path / "cfg").write_text("STARTWORD = !SENT_START\nENDWORD = !SENT_END\nSORTLATTICE = %s\n" % ("T" if run["sort"] else "F"))
    monkeypatch.chdir(tmp_path)
    hlrescore_batch.main(["-C", "cfg"] + run["args"] + ([] if "-i" in run["args"] else ["-l", "out"]) + [G["dict_path"]] + ["in/%s.lat" % n for n in run["lats"]])
    got = {"out/" + f: open(os.path.join("out", f)).read() for f in sorted(os.listdir("out"))}
    if os.path.exists("out.mlf"):
        got["out.mlf"] = open("out.mlf").read()
    assert sorted(got) == sorted(run["files"])
    for f in run["files"]:
        assert got[f] == run["files"][f], f


@pytest.mark.parametrize("g", ["random", "nb_bigram", "big"])
def test_five_settings_in_one_call(native, groups, g):
    """K = 5 in one call = five K = 1 calls = the -T totals of the fixtures."""
    G = groups[g]
    ls = native.LatSet(G["dict_path"], "!SENT_START", "!SENT_END")
    for n in G["names"]:
        ls.add_file(G["paths"][n])
    runs = [next(r for r in RUNS if r["group"] == g and r["name"] == n) for n in F5]
    st = [lu.setting_of(r["args"]) for r in runs]
    all5 = ls.best(st)
    fb5 = ls.fb_max(st)
    for k in range(5):
        one = ls.best([st[k]])
        fb1 = ls.fb_max([st[k]])
        assert np.array_equal(one["totals"][0], all5["totals"][k]) and np.array_equal(one["status"][0], all5["status"][k])
        assert np.array_equal(fb1["best"][0], fb5["best"][k])
        for u, n in enumerate(G["names"]):
            assert np.array_equal(one["paths"][0][u], all5["paths"][k][u])
            assert np.array_equal(fb1["fw"][u][:, 0], fb5["fw"][u][:, k]) and np.array_equal(fb1["bw"][u][:, 0], fb5["bw"][u][:, k])
            assert ["%.3f" % x for x in all5["totals"][k, u]] == runs[k]["totals"][n]


def pick(pool, which):
    """Names from the random groups alone (one dictionary), so that every case is ONE set and one call."""
    small = [n for n in sorted(pool) if pool[n]["lat"]["nArcs"] <= 200 and not n.startswith("rescore")]
    if which == 1:
        return ["r90"]
    if which == 5:
        return ["tile63", "tile64", "tile65", "one", "r90"]
    if which == 70:
        return [small[i % len(small)] for i in range(70)]
    return ["one", "r12", "r31", "tile65", "r90", "big3000"]


@pytest.mark.parametrize("K", [1, 3, 65])
@pytest.mark.parametrize("U", [1, 5, 70, "mixed"])
def test_shapes_against_the_restatement(native, pool, K, U):
    names = pick(pool, U)
    ls = native.LatSet(pool[names[0]]["dict_path"], "!SENT_START", "!SENT_END")
    for n in names:
        ls.add_file(pool[n]["path"])
    assert len(ls) == len(names) == (6 if U == "mixed" else U)   # U = 70, K = 1: 70 pairs, a full block and a partial one
    nn, _ = ls.sizes()
    if U == 5:
        tile = native.latset_tile()
        assert [int(x) <= tile for x in nn] == [True, True, False, True, False]      # both sides of the tile in one call
    st = settings_for(K)
    b, fb = ls.best(st), ls.fb_max(st)
    th = [0.001, 9000.0, 150.0][:K] + [60.0] * max(K - 3, 0)
    aps = [0.0, 0.0, 40.0][:K] + [25.0] * max(K - 3, 0)
    pr = ls.prune(st, th, aps)
    memo = {}
    for u, n in enumerate(names):
        l, o = pool[n]["lat"], pool[n]["orders"]
        for k in range(K):
            if (n, k) not in memo:
                memo[(n, k)] = (lu.find_best(l, o, st[k]), lu.fb_max(l, o, st[k]), lu.prune(l, o, st[k], th[k], aps[k]))
            (path, tot), (fw, bw, best), (kn, ka) = memo[(n, k)]
            assert np.array_equal(b["paths"][k][u], path), (n, k)
            assert np.array_equal(b["totals"][k, u], tot), (n, k)
            assert b["status"][k, u] == (len(path) > 0)
            assert np.array_equal(fb["fw"][u][:, k], fw) and np.array_equal(fb["bw"][u][:, k], bw) and fb["best"][k, u] == best, (n, k)
            assert np.array_equal(pr["keep_node"][k][u], kn) and np.array_equal(pr["keep_arc"][k][u], ka), (n, k)


def test_a_beam_of_zero_with_an_arc_rate_is_refused(native, pool):
    ls = native.LatSet(pool["r12"]["dict_path"], "!SENT_START", "!SENT_END")
    ls.add_file(pool["r12"]["path"])
    with pytest.raises(native.HtkAmdError) as e:
        ls.prune([(1, 1, 0, 1)], 0.0, 40.0)
    assert "beam above zero" in str(e.value)
    assert ls.prune([(1, 1, 0, 1)], 0.0)["keep_arc"][0][0].any()   # without a rate a beam of zero is HLRescore -t 0


def test_prune_flags(native, groups, pool):
    """The tight beam leaves the best path (no route of the rescore lattices ties with it), the wide beam everything, the arcs-per-second limit
    narrows the beam; a pruned lattice scored again gives the same best path."""
    G = groups["rescore"]
    ls = native.LatSet(G["dict_path"], "!SENT_START", "!SENT_END")
    for n in G["names"]:
        ls.add_file(G["paths"][n])
    st = [(1.0, 5.0, -10.5, 1.0)] * 3
    pr = ls.prune(st, [0.001, 9000.0, 150.0], [0.0, 0.0, 40.0])
    best = ls.best(st[:1])
    again = [native.LatSet(like=ls) for _ in range(3)]
    for u, n in enumerate(G["names"]):
        v = ls.view(u)
        path = best["paths"][0][u]
        assert sorted(np.flatnonzero(pr["keep_arc"][0][u])) == sorted(path)
        assert set(np.flatnonzero(pr["keep_node"][0][u])) == {v["start"]} | {int(v["arcEnd"][a]) for a in path}
        assert pr["keep_arc"][1][u].all() and pr["keep_node"][1][u].all()
        assert pr["keep_arc"][2][u].sum() < pr["keep_arc"][1][u].sum()
        for k in range(3):
            again[k].add_pruned(ls, u, pr["keep_node"][k][u], pr["keep_arc"][k][u])
    for k in range(3):
        b2 = again[k].best(st[:1])
        assert np.array_equal(b2["totals"][0], best["totals"][0])
        for u in range(len(ls)):
            old = np.flatnonzero(pr["keep_arc"][k][u])
            assert np.array_equal(old[b2["paths"][0][u]], best["paths"][0][u])


def test_a_decoder_lattice_goes_in_through_latset_add(native, groups):
    """htkamd_latset_add with the arrays of a decoder's lattice (here: a fixture lattice put into that form) scores like the file."""
    G = groups["rescore"]
    case = os.path.join(ROOT, "tests", "golden", "decode", "bigram")
    mmf = native.Mmf([os.path.join(case, "MMF")], hmm_list=os.path.join(case, "hmmlist"))
    net = native.Net(os.path.join(case, "net.slf"), os.path.join(case, "dict"), mmf)
    L = native.lib()
    pron = {(net.word_names[k], int(L.htkamd_net_pron_num(net.h, k))): k for k in range(net.desc.nProns)}
    files, arrays = native.LatSet(G["dict_path"], "!SENT_START", "!SENT_END"), native.LatSet(G["dict_path"], "!SENT_START", "!SENT_END")
    for n in G["names"]:
        l = lu.read_slf(G["paths"][n])
        inv = np.array(l["line"])                                 # latset_add takes the arcs in number order: renumber them by line
        lat = dict(nodeFrame=np.round(l["nodeTime"] * 100).astype(np.int32), nodePron=np.array([pron.get((w, v), -1) for w, v in zip(l["word"], l["var"])], np.int32),
                   nodeLike=np.zeros(l["nNodes"]), arcStart=l["arcStart"][inv], arcEnd=l["arcEnd"][inv], arcAc=l["arcAc"][inv], arcLm=l["arcLm"][inv], arcPr=l["arcPr"][inv],
                   lmScale=1.0, wordPen=0.0, prScale=1.0)
        files.add_file(G["paths"][n]); arrays.add(lat, net)
    st = [(1.0, 5.0, -10.5, 1.0), (0.5, 0.0, 3.25, 1.0)]
    a, b = files.best(st), arrays.best(st)
    assert np.array_equal(a["totals"], b["totals"])
    for k in range(2):
        for u, n in enumerate(G["names"]):
            line = np.array(lu.read_slf(G["paths"][n])["line"])
            assert np.array_equal(line[b["paths"][k][u]], a["paths"][k][u])
    # a PRUNED lattice fed back through htkamd_latset_add and scored again: the same best path, and the same as through add_pruned
    pr = arrays.prune(st[:1], 60.0)
    fed, compacted = native.LatSet(like=arrays), native.LatSet(like=arrays)
    for u in range(len(arrays)):
        kn, ka = pr["keep_node"][0][u], pr["keep_arc"][0][u]
        assert not ka.all()
        v = arrays.view(u)
        renum = np.cumsum(kn) - 1
        fed.add(dict(nodeFrame=np.round(v["nodeTime"][kn] * 100).astype(np.int32), nodePron=np.array([pron.get((arrays.word_name(w), int(x)), -1) for w, x in
                                                                                                         zip(v["nodeWord"][kn], v["nodeVar"][kn])], np.int32),
                     nodeLike=np.zeros(int(kn.sum())), arcStart=renum[v["arcStart"][ka]], arcEnd=renum[v["arcEnd"][ka]], arcAc=v["arcAc"][ka], arcLm=v["arcLm"][ka],
                     arcPr=v["arcPr"][ka], lmScale=1.0, wordPen=0.0, prScale=1.0), net)
        compacted.add_pruned(arrays, u, kn, ka)
    c, d = fed.best(st[:1]), compacted.best(st[:1])
    assert np.array_equal(c["totals"][0], b["totals"][0]) and np.array_equal(d["totals"][0], b["totals"][0])
    for u in range(len(arrays)):
        assert np.array_equal(c["paths"][0][u], d["paths"][0][u])
        assert np.array_equal(np.flatnonzero(pr["keep_arc"][0][u])[c["paths"][0][u]], b["paths"][0][u])


def test_grid_to_scorer(native, groups, tmp_path, capsys):
    """htkamd_latset_best_ids -> htkamd_results_score over a 2 x 2 grid = scoring the four label sets the reference wrote."""
    G = groups["nb_bigram"]
    runs = {r["name"]: r for r in RUNS if r["group"] == "nb_bigram"}
    ls = native.LatSet(G["dict_path"], "!SENT_START", "!SENT_END")
    for n in G["names"]:
        ls.add_file(G["paths"][n])
    grid = [(1.0, s, p, 1.0) for s in (1.0, 5.0) for p in (0.0, -10.5)]
    ref_runs = {(1.0, 0.0): "f_default", (1.0, -10.5): "f_s1_pm10", (5.0, 0.0): "f_s5_p0", (5.0, -10.5): "f_s5_pm10"}
    res = native.Results()
    words = lambda text: [ln.split()[2] for ln in text.splitlines() if len(ln.split()) >= 3]
    truth = [words(runs["f_default"]["files"]["out/%s.rec" % n]) for n in G["names"]]
    refs = [res.add_ref(n, t) for n, t in zip(G["names"], truth)]
    best = ls.best(grid)
    hyps = ls.best_ids(res, best)
    got = res.score(refs, hyps)
    for k, (a, s, p, r) in enumerate(grid):
        files = runs[ref_runs[(s, p)]]["files"]                  # what the reference wrote under this setting
        want = res.score(refs, [[res.ids_of(words(files["out/%s.rec" % n])) for n in G["names"]]])
        assert np.array_equal(got["counts"][k], want["counts"][0]) and np.array_equal(got["totals"][k], want["totals"][0])
        for u, n in enumerate(G["names"]):
            assert [res.label_name(i) for i in hyps[k][u]] == words(files["out/%s.rec" % n])
    assert got["totals"][0][1:4].sum() == 0                        # the references ARE setting 0's paths


def test_the_grid_switch_prints_a_block_per_setting(native, groups, tmp_path, monkeypatch):
    import hlrescore_batch
    G = groups["nb_bigram"]
    runs = {r["name"]: r for r in RUNS if r["group"] == "nb_bigram"}
    mlf = "#!MLF!#\n" + "".join('"*/%s.lab"\n%s.\n' % (n, "".join(ln.split()[2] + "\n" for ln in runs["f_default"]["files"]["out/%s.rec" % n].splitlines())) for n in G["names"])
    (tmp_path / "ref.mlf").write_text(mlf)
    (tmp_path / "cfg").write_text("STARTWORD = !SENT_START\nENDWORD = !SENT_END\n")
    monkeypatch.chdir(tmp_path)
    r = hlrescore_batch.main(["-C", "cfg", "-f", "-l", "out", "--grid", "s=1,5;p=0,-10.5", "-I", "ref.mlf", G["dict_path"]] + [G["paths"][n] for n in G["names"]])
    assert len(r["settings"]) == 4 and r["report"]["totals"].shape[0] == 4
    assert r["report"]["totals"][0][1:4].sum() == 0
    for n in G["names"]:
        assert open("out/k0/%s.rec" % n).read() == runs["f_default"]["files"]["out/%s.rec" % n]
        assert open("out/k3/%s.rec" % n).read() == runs["f_s5_pm10"]["files"]["out/%s.rec" % n]


def test_live_sweep_against_the_reference_binary(native, tmp_path, monkeypatch):
    """Where the reference binary was built: 40 random lattices x 3 settings, -f and -t."""
    exe = os.path.join(ROOT, "oracle", "_ref", "HLRescore")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/HLRescore is not built")
    import random
    import hlrescore_batch
    rng = random.Random(99)
    os.makedirs(str(tmp_path / "in"))
    names = []
    for i in range(40):
        nn = rng.randrange(4, 120)
        names.append("s%d" % i)
        (tmp_path / "in" / ("s%d.lat" % i)).write_text(gen.random_lattice(rng, nn, rng.randrange(nn, 4 * nn), "s%d" % i, i % 2 == 0))
    (tmp_path / "dict").write_text(gen.RAND_DICT)
    (tmp_path / "cfg").write_text("STARTWORD = !SENT_START\nENDWORD = !SENT_END\n")
    for j, args in enumerate((["-f", "-s", "7.5", "-p", "-3.0"], ["-f", "-t", "80.0", "-w", "-s", "3.0", "-p", "2.0", "-r", "0.5"], ["-f", "-t", "200.0", "30.0", "-w", "-a", "0.7"])):
        for who in ("ref", "dev"):
            os.makedirs(str(tmp_path / ("%s%d" % (who, j))))
        cmd = ["-C", "cfg"] + args + ["-l"]
        subprocess.run([exe] + cmd + ["ref%d" % j, "dict"] + ["in/%s.lat" % n for n in names], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL)
        monkeypatch.chdir(tmp_path)
        hlrescore_batch.main(cmd + ["dev%d" % j, "dict"] + ["in/%s.lat" % n for n in names])
        ref = sorted(os.listdir(str(tmp_path / ("ref%d" % j))))
        assert ref == sorted(os.listdir(str(tmp_path / ("dev%d" % j)))) and len(ref) == 40 * (2 if "-w" in args else 1)
        for f in ref:
            assert (tmp_path / ("dev%d" % j) / f).read_text() == (tmp_path / ("ref%d" % j) / f).read_text(), (j, f)
