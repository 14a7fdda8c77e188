"""Label statistics and network arcs on the device: counts and the CSR table against numpy.unique over the same pairs at the shapes where
each kernel can go wrong, the arc kernel against a plain restatement of HBuild's arc order, and the committed cases end to end against the
reference's bytes (tests/golden/lm)."""
import os

import numpy as np
import pytest

from htk_amd import capi
import lm_cases as lc

pytestmark = pytest.mark.gpu

WAVE, GROUP = capi.lib().htkamd_lstats_wave_cap(), capi.lib().htkamd_lstats_group_cap()


def check(V, utts, enter, exit_, times=None, **caps):
    got = capi.lstats_probe(V, utts, enter, exit_, times=times, **caps)
    count, pairs, durs = lc.gather(utts, V, enter, exit_, times)
    rowOff, succ, cnt = lc.csr(pairs, V)
    assert np.array_equal(got["count"], count)
    assert np.array_equal(got["rowOff"], rowOff) and np.array_equal(got["succ"], succ) and np.array_equal(got["cnt"], cnt)
    if times is not None:
        for w in range(V):
            if w in durs:
                assert (got["durSum"][w], got["durMin"][w], got["durMax"][w]) == (sum(durs[w]), min(durs[w]), max(durs[w])), w
            else:
                assert got["durSum"][w] == 0 and got["durMin"][w] == np.iinfo(np.int64).max and got["durMax"][w] == np.iinfo(np.int64).min
    return got


def row_of(pred, n_distinct, first=2, repeat=1):
    """Utterances `pred w` for n_distinct words w, each `repeat` times: a row of pred with exactly n_distinct successors."""
    return [np.array([pred, first + k], np.int32) for k in range(n_distinct) for _ in range(repeat)]


def test_empty_batch():
    got = capi.lstats_probe(5, [], 1, 4)
    assert not got["count"].any() and not got["rowOff"].any() and len(got["succ"]) == 0


@pytest.mark.parametrize("utts", [[[]], [[], [3]], [[3]], [[1, 3, 4]], [[1], [4]], [[3, 1, 2, 4, 3]], [[0, 3, 0]]], ids=str)
def test_boundaries(utts):
    """no label (the boundary pair alone), one label, the boundary words at the edges (skipped) and in mid-sentence (counted, no bigram),
    a label outside the list (id 0)"""
    check(5, [np.array(u, np.int32) for u in utts], 1, 4)


def test_one_word_vocabulary():
    check(3, [np.array([], np.int32), np.array([], np.int32)], 1, 2)      # the two boundary words and the null slot: nothing else can be said
    check(4, [np.array([2, 2, 2], np.int32), np.array([2], np.int32)], 1, 3)


@pytest.mark.parametrize("n", [63, 64, 65, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1])
def test_row_lengths_around_the_paths(n):
    """a row with n distinct successors: the lanes of a wavefront, the wavefront path's capacity, the workgroup path's"""
    V = n + 4
    got = check(V, row_of(2, n, first=3), 1, V - 1)
    assert got["rowOff"][3] - got["rowOff"][2] == n


@pytest.mark.parametrize("wave,group", [(4, 4), (4, 8), (3, 5), (1, 1)])
def test_small_capacities_force_every_path(wave, group):
    """rows of 1..12 pairs under capacities of a few pairs: the wavefront path, the workgroup path and the histogram path (windows of
    `group` ids, several of them) all run, in a table of 16 words"""
    rng = np.random.default_rng(5)
    utts = [rng.integers(0, 16, rng.integers(0, 9)).astype(np.int32) for _ in range(40)]
    check(16, utts, 1, 15, wave_cap=wave, group_cap=group)


def test_every_pair_identical_and_every_pair_distinct():
    got = check(6, [np.array([2, 3], np.int32)] * 3000, 1, 5)          # runs of maximal length: one entry per row
    assert list(got["cnt"]) == [3000, 3000, 3000]
    V = 300
    check(V, [np.array([2 + (k % 290), 2 + (k // 290)], np.int32) for k in range(290 * 4)], 1, V - 1)


def test_ids_at_both_ends():
    V = 70
    check(V, [np.array([0, V - 2, 0, V - 2], np.int32), np.array([V - 2], np.int32), np.array([V - 1, 2, 1], np.int32)], 1, V - 1)
    check(V, [np.array([V - 1, 2], np.int32)], V - 1, 0)              # the boundary words at the other ends of the table


def test_durations():
    utts = [np.array([2, 3, 2], np.int32), np.array([2, 4], np.int32)]
    times = [np.array([[0, 50], [50, 80], [80, 130]], np.int64), np.array([[0, 50], [7, 7]], np.int64)]      # equal durations, a single one, zero
    check(6, utts, 1, 5, times=times)


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(9)
    utts = [rng.zipf(1.3, rng.integers(1, 40)).clip(0, 499).astype(np.int32) for _ in range(400)]
    a, b = capi.lstats_probe(500, utts, 1, 499), capi.lstats_probe(500, utts, 1, 499)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    check(500, utts, 1, 499)


def arcs_plain(mode, N, nodeOf, rowKeep, enter, zap, rowOff, succ, val, rowVal, uni):
    """ProcessBoBiGram's / ProcessMatBiGram's loops (HBuild.c:409-458, :502-516) in plain Python"""
    out = []
    if mode == capi.LM_BACKOFF:
        out += [(0, nodeOf[i], uni[i]) for i in range(1, N + 1) if nodeOf[i] >= 0 and i != enter]
        for i in range(1, N + 1):
            if rowKeep[i]:
                out.append((nodeOf[i], 0, rowVal[i]))
                out += [(nodeOf[i], nodeOf[s], val[t]) for t in range(rowOff[i], rowOff[i + 1]) for s in [succ[t]] if nodeOf[s] >= 0 and s != enter]
    else:
        for i in range(1, N):
            if rowKeep[i]:
                out += [(nodeOf[i], nodeOf[j], val[i * (N + 1) + j]) for j in range(2, (N - 1 if i == 1 else N) + 1) if j != zap]
    return out


@pytest.mark.parametrize("N,zap", [(5, 0), (70, 0), (70, 33), (130, 2)])
def test_arc_kernel_against_the_plain_loops(N, zap):
    rng = np.random.default_rng(N + zap)
    nodeOf, j = np.full(N + 1, -1, np.int32), 1
    for i in range(1, N + 1):
        if i != zap:
            nodeOf[i] = j; j += 1
    rowKeep = np.array([0] + [int(i != zap and i != N) for i in range(1, N + 1)], np.int32)
    lens = np.minimum(rng.integers(0, 9, N + 1), N); lens[0] = 0; lens[min(3, N)] = 0; lens[2] = N      # an empty row and a full one
    rows = [np.sort(rng.choice(np.arange(1, N + 1), lens[i], replace=False)) for i in range(N + 1)]
    rowOff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)      # (row 0 is empty: rows 1..N start at rowOff[1] = 0)
    succ = np.concatenate(rows).astype(np.int32)
    val, rowVal, uni = rng.standard_normal(len(succ)).astype(np.float32), rng.standard_normal(N + 1).astype(np.float32), rng.standard_normal(N + 1).astype(np.float32)
    S, E, L = capi.netbuild_probe(capi.LM_BACKOFF, N, nodeOf, rowKeep, 1, zap, rowOff=rowOff, succ=succ, val=val, rowVal=rowVal, uni=uni)
    want = arcs_plain(capi.LM_BACKOFF, N, nodeOf, rowKeep, 1, zap, rowOff, succ, val, rowVal, uni)
    assert list(zip(S, E)) == [(a, b) for a, b, _ in want] and L.tobytes() == np.array([v for _, _, v in want], np.float32).tobytes()
    mat = rng.standard_normal((N + 1) * (N + 1)).astype(np.float32)
    nodeM = np.where(nodeOf >= 0, nodeOf - 1, -1).astype(np.int32)
    S, E, L = capi.netbuild_probe(capi.LM_MATRIX, N, nodeM, rowKeep, 1, zap, val=mat)
    want = arcs_plain(capi.LM_MATRIX, N, nodeM, rowKeep, 1, zap, None, None, mat, None, None)
    assert list(zip(S, E)) == [(a, b) for a, b, _ in want] and L.tobytes() == np.array([v for _, _, v in want], np.float32).tobytes()


@pytest.mark.parametrize("case,name", lc.variants())
def test_committed_cases_end_to_end(case, name, tmp_path):
    """labels -> device counts -> bigram file and listings; the reference's bigram file -> network -> SLF: all the reference's bytes"""
    d, words, utts, manifest = lc.load_case(case)
    spec = manifest[name]
    if spec["hlstats"] is not None:
        enter, exit_ = lc.boundary(spec)
        ls = capi.LabelStats(words, enter, exit_)
        ids, times = lc.case_ids(ls, utts)
        ls.count(ids, times)
        for suffix, data in lc.run_variant(capi, ls, spec, str(tmp_path), name).items():
            assert data == open(os.path.join(d, name + "." + suffix), "rb").read(), suffix
    if spec["hbuild"] is not None:
        _, data = lc.build_net(capi, d, words, name, spec, str(tmp_path))
        assert data == open(os.path.join(d, name + ".slf"), "rb").read()


def test_example_finds_label_files_as_hlstats_does(tmp_path):
    """examples/hlstats_bigram.py over the toy case as single label files: named directly, through -L dir -X ext, and through -I mlf"""
    import subprocess, sys
    d, words, utts, manifest = lc.load_case("toy")
    labs = tmp_path / "labs"; labs.mkdir()
    names = []
    for k, u in enumerate(utts):
        (labs / ("u%03d.lab" % k)).write_text("".join("%d %d %s\n" % (s, e, w) for w, s, e in u))
        names.append("u%03d" % k)
    ex = os.path.join(os.path.dirname(lc.GOLD), "..", "..", "examples", "hlstats_bigram.py")
    want = open(os.path.join(d, "bo.bigram"), "rb").read()
    for sw, files in (([], [str(labs / (n + ".lab")) for n in names]),
                      (["-L", str(labs), "-X", "lab"], ["/data/%s.rec" % n for n in names]),
                      (["-I", os.path.join(d, "labels.mlf")], ["/nowhere/%s.lab" % n for n in names])):
        out = tmp_path / "bo"
        r = subprocess.run([sys.executable, ex, "-o", "-b", str(out)] + sw + [os.path.join(d, "wordlist")] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert out.read_bytes() == want, sw
