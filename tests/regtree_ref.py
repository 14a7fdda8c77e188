"""A sequential float32 restatement of the regression class tree's device steps (htk_amd/csrc/regtree.hip), written from the reference's
HHEd.c as read: Distance (:5657), CalcDistance (:5863), CalcClusterDistribution (:5692), CalcNodeScore (:5673), CreateChildNodes (:5912)
and ClusterChildren's loop (:5961, thresh = 1e-12f, MAX_ITER = 500); and of the host's part, BuildRegClusters (:6096) with
FindBestTerminal (:6073) and PerturbMean (:5850), to step a whole RC command.

One float32 operation at a time, nothing fused.  A sum over members is np.add.accumulate(dtype=float32) over the selected rows in list
order, started from +0 as the C sums are; the square root is the double's, rounded to float32.  A member with has == 0 is assigned and
partitioned and enters no sum; a tie or a NaN sends a member right.  Callers wrap the calls in np.errstate(all="ignore"): an empty child's
figures are 0 / 0.

tests/test_regtree_ref.py pins this file to HHEd's recorded trees; tests/test_gpu_regtree_kernels.py pins the kernels to it, bit for bit."""
import numpy as np

F = np.float32
THRESH = F(1.0e-12)
MAX_ITER = 500


def chain(rows):
    """The float32 sum of rows[0], rows[1], ... in that order, from +0 (per column)."""
    rows = np.asarray(rows, F)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + rows.shape[1:], F), rows]), axis=0, dtype=F)[-1]


def distance(m, c):
    """Distance of every row of m[n, D] to c[D]: the squares summed over k = 1..D in float32, the root of the double."""
    x = m - c
    x = x * x
    dist = np.add.accumulate(x, axis=1, dtype=F)[:, -1]
    return np.sqrt(dist.astype(np.float64)).astype(F)


def perturb(mean, covar, depth):
    return mean + F(depth) * covar


class RegTreeRef:
    """The member arrays and the member list; node() and split() as the device's steps, on list[off : off + n]."""

    def __init__(self, mean, sum, sqr, occ, has):
        self.mean, self.sum, self.sqr = (np.ascontiguousarray(a, F) for a in (mean, sum, sqr))
        self.occ = np.ascontiguousarray(occ, F)
        self.has = np.asarray(has) != 0
        self.G, self.D = self.mean.shape
        self.list = np.arange(self.G, dtype=np.int32)

    def _node(self, ids):
        """aveMean[D], aveCovar[D], clustAcc, clusterScore of the members ids, in that order."""
        h = self.has[ids]
        acc = ids[h]
        s, q, occ = chain(self.sum[acc]), chain(self.sqr[acc]), chain(self.occ[acc])
        mean = s / occ
        covar = (q - (s * s) / occ) / occ
        score = chain((distance(self.mean[ids], mean) * self.occ[ids])[h])
        return np.concatenate([mean, covar, [occ, score]]).astype(F)

    def node(self, off, n):
        return self._node(self.list[off:off + n])

    def _assign(self, ids, cen):
        s1, s2 = distance(self.mean[ids], cen[0]), distance(self.mean[ids], cen[1])
        left = s1 < s2
        return left, self.occ[ids] * np.where(left, s1, s2)

    def split(self, off, n, seeds):
        """(counts int32[3] = members left, right, CalcDistance calls; float32[2, 2D+2] = the children); the list is partitioned."""
        ids = self.list[off:off + n].copy()
        h = self.has[ids]
        cen = np.array(seeds, F).reshape(2, self.D)
        it = calls = 0
        new = F(0.0)
        while True:
            it += 1
            if it >= MAX_ITER:
                break
            left, val = self._assign(ids, cen)
            calls += 1
            L, R = left & h, ~left & h
            a1, a2 = chain(self.occ[ids[L]]), chain(self.occ[ids[R]])
            c1, c2 = chain(val[L]), chain(val[R])
            cen = np.stack([chain(self.sum[ids[L]]) / a1, chain(self.sum[ids[R]]) / a2])
            d = (c1 + c2) / (a1 + a2)
            old = (d + THRESH) + F(1.0) if it == 1 else new
            new = d
            if not (old - new > THRESH):
                break
        left, _ = self._assign(ids, cen)
        self.final_centroids = cen                       # what CreateChildNodes assigns against
        l, r = ids[left], ids[~left]
        self.list[off:off + n] = np.concatenate([l, r])
        return np.array([l.size, r.size, calls], np.int32), np.stack([self._node(l), self._node(r)])


def run_steps(ref, steps):
    """The steps of capi.regtree_probe over a RegTreeRef, with its results: (results, list)."""
    out = []
    with np.errstate(all="ignore"):
        for st in steps:
            out.append(ref.node(st[1], st[2]) if st[0] == "node" else ref.split(st[1], st[2], st[3]))
    return out, ref.list.copy()


def build_tree(ref, n_terminals, n_nonspeech=0):
    """A whole RC command over the members (the first n_nonspeech of them RC's item list): the root node(s), then BuildRegClusters.
    Returns (steps, results, kids, ranges): the device steps in the order they are made with their results, the children (left, right) of
    node 1, 2, ... ((0, 0): a terminal) and every node's (off, n) in the final list."""
    D, G = ref.D, ref.G
    nd = {}

    def new(off, n):
        return dict(left=0, right=0, off=off, n=n, dist=None, score=F(0.0))

    def take(t, fig):
        nd[t]["dist"], nd[t]["score"] = fig, fig[2 * D + 1]

    steps, results = [], []
    root_split = n_nonspeech > 0
    splits = (2 if root_split else 1) < n_terminals
    with np.errstate(all="ignore"):
        if root_split:
            nd[1] = new(0, 0); nd[1]["left"], nd[1]["right"] = 2, 3
            nd[2], nd[3] = new(0, n_nonspeech), new(n_nonspeech, G - n_nonspeech)
            for i in ((3, 2) if splits else ()):
                steps.append(("node", nd[i]["off"], nd[i]["n"])); results.append(ref.node(nd[i]["off"], nd[i]["n"])); take(i, results[-1])
            index = 4
        else:
            nd[1] = new(0, G)
            if splits:
                steps.append(("node", 0, G)); results.append(ref.node(0, G)); take(1, results[-1])
            index = 2

        def find_best(t, score, best):
            if nd[t]["left"]:
                score, best = find_best(nd[t]["left"], score, best)
                score, best = find_best(nd[t]["right"], score, best)
            elif score < nd[t]["score"] and nd[t]["n"] > D * 3:
                score, best = nd[t]["score"], t
            return score, best

        for k in range(index // 2, n_terminals):
            score, t = find_best(1, F(0.0), 1)
            if (k > 1 or score == 0.0) and t == 1:
                break
            fig = nd[t]["dist"]
            seeds = np.stack([perturb(fig[:D], fig[D:2 * D], 0.2), perturb(fig[:D], fig[D:2 * D], -0.2)])
            steps.append(("split", nd[t]["off"], nd[t]["n"], seeds))
            counts, two = ref.split(nd[t]["off"], nd[t]["n"], seeds)
            results.append((counts, two))
            for c in range(2):
                nd[index] = new(nd[t]["off"] + (int(counts[0]) if c else 0), int(counts[c]))
                take(index, two[c])
                nd[t]["right" if c else "left"] = index
                index += 1
    kids = [(nd[i]["left"], nd[i]["right"]) for i in range(1, index)]
    return steps, results, kids, [(nd[i]["off"], nd[i]["n"]) for i in range(1, index)]
