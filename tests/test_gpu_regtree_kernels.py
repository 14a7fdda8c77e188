"""The regression class tree's kernels themselves (htk_amd/csrc/regtree.hip: k_rt_node, k_rt_split), through the test aid
capi.regtree_probe, against the sequential float32 restatement tests/regtree_ref.py (which tests/test_regtree_ref.py pins to HHEd):
every figure a step returns -- both children's means, covariances, occupation and score, the counts with the number of CalcDistance
calls -- and the member list, bit for bit.  The one exception: where the restatement's value is a NaN (0 / 0 of a child without
occupation) the device's must be a NaN too; sign and payload of 0 / 0 are the machine's.

The shapes are the smallest that reach the code the recorded cases (at most 480 members, D <= 7) never run:
    n = 1 .. 130 at D = 5      the tail loops of the four ordered walks alone (n < 16), n either side of a multiple of 16 and of a wavefront
    n = 1023 .. 3000 at D = 3  the second and third pass of the partition loop and of every stride loop (1024 threads)
    D = 39                     the project's vector size, below and above one pass
    D = 1 .. 129 at n = 200    the occupation lane at thread 64, 128 and 192: dimension lanes across wavefronts (D = 63 / 64 / 65, 128 / 129)
    D = 960 at n = 40          the largest vector size the device state accepts
Per shape: the root's node step and split, the right child's node step and split (a range at off > 0 of a permuted list), the left
child's split; a child is split when it has at least 2 members.  The seeds are the node's mean +- 0.2 covariance, as the host makes them.
Further sets: five that split evenly (BALANCED), cases of their own (an empty child, members without a record, one member, an exact tie)
and the mirror sets, which make the order of the LOOP's centroid sums show -- no step returns those."""
import functools
import time

import numpy as np
import pytest

import regtree_ref as rr

F = np.float32

SHAPES = ([(n, 5) for n in (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 130)] + [(n, 3) for n in (1023, 1024, 1025, 2049, 3000)] + [(200, 39), (1025, 39)]
          + [(200, D) for D in (1, 63, 64, 65, 128, 129)] + [(40, 960)])
# With magnitudes that far apart a split is often a few members against the rest.  The same code once more over means drawn around four
# centres (as the recorded case h's are), where a split is balanced: left and right members interleave through every pass of the partition.
BALANCED = [(130, 5), (1025, 3), (3000, 3), (1025, 39), (200, 65)]


def make_members(n, D, seed, centres=0):
    """mean, sum, sqr, occ, has: magnitudes that differ per member (the order of the adds shows) or, with centres > 0, means around that
    many centres; occupations in (0, 50], about a tenth of the members without an AccSum record (has = 0, occupation 0, zero rows), a few
    pairs with identical means."""
    rng = np.random.RandomState(seed)
    if centres:
        mean = (3.0 * rng.randn(centres, D)[rng.randint(0, centres, n)] + 2.7 * rng.randn(n, D)).astype(F)
    else:
        mean = (rng.randn(n, D) * np.exp(3.0 * rng.randn(n, 1))).astype(F)
    for _ in range(min(3, n // 8)):
        a, b = rng.randint(0, n, 2)
        mean[b] = mean[a]
    var = (0.5 + rng.rand(n, D)).astype(F)
    occ = (50.0 * (1.0 - rng.rand(n))).astype(F)
    has = rng.rand(n) >= 0.1
    has[0] = True
    occ[~has] = 0.0
    sum_ = mean * occ[:, None]                                   # host/regtree.c:338, a float product each
    sqr = (var + mean * mean) * occ[:, None]
    assert sum_.dtype == F and sqr.dtype == F and (occ[has] > 0).all()
    return mean, sum_, sqr, occ, has.astype(np.uint8)


def seeds_of(fig, D):
    return np.stack([rr.perturb(fig[:D], fig[D:2 * D], 0.2), rr.perturb(fig[:D], fig[D:2 * D], -0.2)])


def usual_steps(ref, n):
    """The steps of a shape, made and answered by the restatement: (steps, results, list)."""
    D = ref.D
    steps, results = [], []

    def do(step):
        steps.append(step)
        results.append(ref.node(step[1], step[2]) if step[0] == "node" else ref.split(step[1], step[2], step[3]))
        return results[-1]

    with np.errstate(all="ignore"):
        root = do(("node", 0, n))
        counts, two = do(("split", 0, n, seeds_of(root, D)))
        nL, nR = int(counts[0]), int(counts[1])
        right = do(("node", nL, nR))
        if nR >= 2:
            do(("split", nL, nR, seeds_of(right, D)))
        if nL >= 2:
            do(("split", 0, nL, seeds_of(two[0], D)))
    return steps, results, ref.list.copy()


@functools.lru_cache(maxsize=None)
def shape_case(n, D, centres=0):
    """(member arrays, steps, the restatement's results and final list) of a shape; computed once, read by every test."""
    arrays = make_members(n, D, seed=7000 + 31 * n + D, centres=centres)
    steps, results, lst = usual_steps(rr.RegTreeRef(*arrays), n)
    for a in arrays + (lst,):
        a.setflags(write=False)
    return arrays, steps, results, lst


def same_floats(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), "%s: the restatement has a NaN where the device has %s" % (what, got[nan][~np.isnan(got[nan])][:4])
    bad = np.flatnonzero(got[~nan].view(np.uint32) != want[~nan].view(np.uint32))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %d: device %r, restatement %r" % (what, bad.size, got.size, bad[0], got[~nan][bad[0]], want[~nan][bad[0]])


def same_results(got, want, got_list, want_list, steps):
    assert len(got) == len(want) == len(steps)
    for s, (st, g, w) in enumerate(zip(steps, got, want)):
        what = "step %d %s(%d, %d)" % (s, st[0], st[1], st[2])
        if st[0] == "split":
            assert np.array_equal(g[0], w[0]), "%s: counts %s, restatement %s" % (what, g[0], w[0])
            same_floats(g[1][0], w[1][0], what + " left child")
            same_floats(g[1][1], w[1][1], what + " right child")
        else:
            same_floats(g, w, what)
    assert np.array_equal(got_list, want_list), "the member list differs"


def test_inputs_exercise_the_split():
    """No device: in at least 90 % of the shapes the restatement's first split gives two non-empty children after more than one
    CalcDistance call (n = 1 cannot) -- else the comparison below would look at little."""
    good = 0
    for n, D in SHAPES:
        _, steps, results, _ = shape_case(n, D)
        counts = results[1][0]
        good += bool(counts[0] > 0 and counts[1] > 0 and counts[2] > 1)
        print("n=%d D=%d: first split %s, %d steps" % (n, D, counts.tolist(), len(steps)))
    assert good >= 0.9 * len(SHAPES), good
    # the balanced sets: every step happens, both children of the first split hold an eighth of the members at least, and the right child
    # is a range at off > 0 of a list that the first split permuted
    for n, D in BALANCED:
        _, steps, results, lst = shape_case(n, D, 4)
        counts = results[1][0]
        print("n=%d D=%d balanced: splits %s" % (n, D, [r[0].tolist() for r in results if isinstance(r, tuple)]))
        assert len(steps) == 5 and min(counts[:2]) >= n // 8 and counts[2] > 2 and steps[2][1] == counts[0] and not np.array_equal(lst[:n], np.arange(n))
    assert shape_case(3000, 3, 4)[1][2][2] > 1024                        # ... beyond one pass of the workgroup


@pytest.mark.gpu
@pytest.mark.parametrize("n,D,centres", [s + (0,) for s in SHAPES] + [s + (4,) for s in BALANCED])
def test_steps_equal_the_restatement(native, n, D, centres):
    arrays, steps, want, want_list = shape_case(n, D, centres)
    t0 = time.time()
    got, got_list = native.regtree_probe(*arrays, steps)
    print("n=%d D=%d: %d steps, splits %s, probe %.3f s" % (n, D, len(steps), [w[0].tolist() for w in want if isinstance(w, tuple)], time.time() - t0))
    same_results(got, want, got_list, want_list, steps)


@pytest.mark.gpu
def test_equal_seeds_leave_the_left_child_empty(native):
    """Every member ties and goes right: counts (0, n), the list as it was, the left child's mean and covariance 0 / 0 on both sides."""
    n, D = 150, 5
    arrays = make_members(n, D, seed=11)
    seed = arrays[0][3].copy()
    steps = [("split", 0, n, np.stack([seed, seed])), ("node", 0, n)]
    with np.errstate(all="ignore"):
        want, want_list = rr.run_steps(rr.RegTreeRef(*arrays), steps)
    counts, two = want[0]
    assert counts[0] == 0 and counts[1] == n and np.array_equal(want_list, np.arange(n))
    assert np.isnan(two[0][:2 * D]).all() and not np.isnan(two[1]).any()
    assert np.array_equal(two[1].view(np.uint32), want[1].view(np.uint32))      # the right child is the whole node
    got, got_list = native.regtree_probe(*arrays, steps)
    assert np.isnan(got[0][1][0][:2 * D]).all()
    same_results(got, want, got_list, want_list, steps)


@pytest.mark.gpu
def test_a_range_without_any_accsum_record(native):
    """Members 20 .. 50 have has = 0: their node is 0 / 0 with occupation and score +0, their split assigns and partitions them and sums
    nothing; a split of the whole list around them still agrees."""
    n, D = 60, 5
    mean, sum_, sqr, occ, has = make_members(n, D, seed=12)
    has[20:50] = 0; occ[20:50] = 0.0; sum_[20:50] = 0.0; sqr[20:50] = 0.0
    arrays = (mean, sum_, sqr, occ, has)
    ref = rr.RegTreeRef(*arrays)
    with np.errstate(all="ignore"):
        root = ref.node(0, n)
    steps = [("node", 20, 30), ("split", 20, 30, np.stack([mean[22], mean[41]])), ("node", 0, n), ("split", 0, n, seeds_of(root, D))]
    want, want_list = rr.run_steps(rr.RegTreeRef(*arrays), steps)
    assert np.isnan(want[0][:2 * D]).all() and want[0][2 * D] == 0 and want[0][2 * D + 1] == 0
    assert want[1][0][0] + want[1][0][1] == 30 and want[3][0][0] > 0 and want[3][0][1] > 0
    got, got_list = native.regtree_probe(*arrays, steps)
    same_results(got, want, got_list, want_list, steps)


@pytest.mark.gpu
def test_rows_of_a_member_without_a_record_enter_no_sum(native):
    """The host gives a member without an AccSum record an occupation of 0 and zero rows, so adding them by mistake would not show in
    the sets above.  Here a third of the members have has = 0 over an occupation and rows that are not zero: no figure may move."""
    n, D = 300, 5
    mean, sum_, sqr, occ, has = make_members(n, D, seed=15, centres=3)
    keep = has.copy()
    has[np.random.RandomState(16).rand(n) < 0.33] = 0
    has[0] = 1
    arrays = (mean, sum_, sqr, occ, has)
    assert (occ[(has == 0) & (keep == 1)] > 0).sum() > 50
    steps, want, want_list = usual_steps(rr.RegTreeRef(*arrays), n)
    assert len(steps) == 5 and min(want[1][0][:2]) > n // 8
    got, got_list = native.regtree_probe(*arrays, steps)
    same_results(got, want, got_list, want_list, steps)


@pytest.mark.gpu
def test_probe_refuses_what_the_device_steps_refuse(native):
    """A range outside the members and a split of no member, before anything is launched."""
    arrays = make_members(8, 3, seed=14)
    zero = np.zeros((2, 3), F)
    for steps in ([("node", 4, 5)], [("node", -1, 2)], [("node", 0, -1)], [("split", 0, 0, zero)], [("split", 7, 2, zero)], [("node", 0, 8), ("split", 8, 1, zero)]):
        with pytest.raises(native.HtkAmdError) as e:
            native.regtree_probe(*arrays, steps)
        assert "range" in str(e.value), steps


@pytest.mark.gpu
def test_one_member(native):
    mean, sum_, sqr, occ, has = make_members(4, 7, seed=13)
    steps = [("node", 2, 1), ("split", 2, 1, np.stack([mean[2] + F(1.0), mean[2] - F(0.5)])), ("node", 2, 1), ("node", 3, 0)]
    want, want_list = rr.run_steps(rr.RegTreeRef(mean, sum_, sqr, occ, has), steps)
    assert want[1][0][:2].tolist() == [0, 1] and np.isnan(want[3][:14]).all()
    got, got_list = native.regtree_probe(mean, sum_, sqr, occ, has, steps)
    same_results(got, want, got_list, want_list, steps)


def dyadic_members(seed=5, pairs=24, D=3):
    """As write_set(dyadic=True): means k / 8 in mirrored pairs (m, -m) behind one another, variances k / 8 and occupations powers of
    two shared by a pair, so the root's mean is exactly 0 and both seeds, then both centroids of every iteration, are mirror images; and
    two members at exactly 0 at the end of the list, without an AccSum record: with one they would go right and weigh on that side."""
    rng = np.random.RandomState(seed)
    m = np.round(rng.randn(pairs, D) * 3.0 * 8.0) / 8.0
    v = np.round((0.5 + rng.rand(pairs, D)) * 8.0) / 8.0
    o = 2.0 ** rng.randint(1, 5, size=pairs)
    mean = np.concatenate([np.stack([m, -m], axis=1).reshape(2 * pairs, D), np.zeros((2, D))]).astype(F)
    var = np.concatenate([np.repeat(v, 2, axis=0), np.ones((2, D))]).astype(F)
    occ = np.concatenate([np.repeat(o, 2), [0.0, 0.0]]).astype(F)
    has = np.ones(2 * pairs + 2, np.uint8); has[-2:] = 0
    return mean, mean * occ[:, None], (var + mean * mean) * occ[:, None], occ, has


@pytest.mark.gpu
def test_a_member_equidistant_from_both_final_centroids(native):
    arrays = dyadic_members()
    n, D = arrays[0].shape
    ref = rr.RegTreeRef(*arrays)
    with np.errstate(all="ignore"):
        root = ref.node(0, n)
        assert not root[:D].any()                                      # the root's mean is exactly 0
        steps = [("node", 0, n), ("split", 0, n, seeds_of(root, D))]
        counts, two = ref.split(*steps[1][1:])
        cen = ref.final_centroids
        d1, d2 = rr.distance(arrays[0][-2:], cen[0]), rr.distance(arrays[0][-2:], cen[1])
    assert np.array_equal(d1, d2) and d1[0] > 0 and counts[0] > 0 and counts[2] > 1      # exact ties against the FINAL centroids
    assert set(ref.list[counts[0]:].tolist()) >= {n - 2, n - 1}                          # ... and a tie goes right
    want, want_list = rr.run_steps(rr.RegTreeRef(*arrays), steps)
    got, got_list = native.regtree_probe(*arrays, steps)
    same_results(got, want, got_list, want_list, steps)


def mirror_case(n_many, D, seed, many_left):
    """A split whose outcome hangs on the last bit of the loop's centroid sums, which no step returns.  n_many members with positive
    means of mixed magnitude are one child, with the centroid c = (their sums in list order) / (their occupations in list order); the other
    child is ONE member at exactly -c with the occupation 8, so its centroid is -c bit for bit; the seeds are (c, -c) -- or all of it
    mirrored, the many on the right.  A last member at 0 without an AccSum record is then exactly as far from one centroid as from the
    other and goes right.  Were the sums made in any order that moves a bit of c, that member would be nearer to the smaller of the two
    centroids: it goes left where the many are left and c shrank, or where the many are right and c grew -- so each set is run both ways."""
    rng = np.random.RandomState(seed)
    x = ((np.abs(rng.randn(n_many, D)) + 0.1) * np.exp(2.0 * rng.randn(n_many, 1))).astype(F)
    occ = (50.0 * (1.0 - rng.rand(n_many))).astype(F)
    order = rng.permutation(n_many + 2)
    rank = np.argsort(order)                                                    # member j of (many, single, zero) stands at rank[j]
    many = np.sort(rank[:n_many])                                               # ... and the many are summed in list order
    mean = np.zeros((n_many + 2, D), F); o = np.zeros(n_many + 2, F); has = np.ones(n_many + 2, np.uint8)
    mean[rank[:n_many]] = x; o[rank[:n_many]] = occ
    c = rr.chain((mean * o[:, None])[many]) / rr.chain(o[many])
    mean[rank[n_many]] = -c; o[rank[n_many]] = 8.0
    has[rank[n_many + 1]] = 0
    if not many_left:
        mean = -mean
    var = (0.5 + rng.rand(n_many + 2, D)).astype(F)
    arrays = (mean, mean * o[:, None], (var + mean * mean) * o[:, None], o, has)
    shows = not np.array_equal(rr.chain(arrays[1][many]), rr.chain(arrays[1][many[::-1]]))
    return arrays, [("split", 0, n_many + 2, np.stack([c, -c]))], int(rank[n_many + 1]), shows


MIRRORS = [(n_many, D, many_left) for n_many in (3, 14, 17, 30, 45, 77, 150) for D in (1, 2) for many_left in (True, False)]


def test_mirror_sets_hang_on_the_order_of_the_sums():
    """No device: in every mirror set the restatement ends with exact mirror centroids, the member at 0 on the right after 2 CalcDistance
    calls; and in three quarters of them at least (the small ones may sum alike) the sum of the many in the opposite order is another float."""
    shown = 0
    for n_many, D, many_left in MIRRORS:
        arrays, steps, zero, shows = mirror_case(n_many, D, 9000 + 7 * n_many + D, many_left)
        ref = rr.RegTreeRef(*arrays)
        (counts, two), = rr.run_steps(ref, steps)[0]
        assert np.array_equal(ref.final_centroids[0], -ref.final_centroids[1]) and np.array_equal(ref.final_centroids, steps[0][3])
        assert counts.tolist() == ([n_many, 2, 2] if many_left else [1, n_many + 1, 2]) and zero in ref.list[counts[0]:]
        shown += shows
    assert shown >= 0.75 * len(MIRRORS), shown


@pytest.mark.gpu
@pytest.mark.parametrize("n_many,D,many_left", MIRRORS)
def test_loop_centroids_keep_list_order(native, n_many, D, many_left):
    arrays, steps, zero, _ = mirror_case(n_many, D, 9000 + 7 * n_many + D, many_left)
    want, want_list = rr.run_steps(rr.RegTreeRef(*arrays), steps)
    got, got_list = native.regtree_probe(*arrays, steps)
    same_results(got, want, got_list, want_list, steps)


@pytest.mark.gpu
def test_recorded_cases_step_by_step(native):
    """The nine recorded cases' own steps (tests/golden/regtree/*/steps.npz): every figure of every step, not only the files they end in."""
    import regtree_util as ru
    from test_regtree_ref import load_case
    for name in sorted(ru.CASES):
        ref, steps, z = load_case(name)
        want, want_list = rr.run_steps(ref, steps)
        got, got_list = native.regtree_probe(z["mean"], z["sum"], z["sqr"], z["occ"], z["has"], steps)
        same_results(got, want, got_list, want_list, steps)
