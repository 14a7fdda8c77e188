#!/usr/bin/env python3
"""Known answers for htkamd_results_* from the reference's HResults (oracle/_ref/HResults), run inside tests/golden/results/ so that the
file names it prints are relative ones:
    HResults [run's switches] list <hypotheses>     -> <run>.out (its whole standard output)
The label sets (words a..e, "sil" as the null class of the -z run; everything seeded):
    corner.ref.mlf / corner.rec.mlf   the places where the alignment kernel can go wrong, a pair each:
        (no empty transcription: the reference's label reader gives an empty file NO label list and HResults then stops with
         "ERROR [+6570] GetLabelList: n[1] > numLists[0]", for an empty reference and an empty hypothesis alike, so it has no answer
         to record; tests/test_gpu_results.py checks those pairs against the grid's edge cells instead)
        one_*              lengths 1 against 1 (hit, substitution) and 1 against 130 both ways
        w63, w64, w65      a reference of 63 / 64 / 65 labels against 64 (the wavefront's edge), and 64 against 65 (w64r)
        long               the only pair whose grid exceeds the kernel's LDS `dir` tile (RES_DIR_TILE of csrc/results.hip): global scratch
        tie_*              ties: a run of one word against a shorter / longer run of it (d == h == v), a substitution beside an insertion
                           and beside a deletion (two-way ties in both orders), a crossed pair
        nul_*              "sil" at the start, at the end, doubled, facing each other, and a pair of nothing but "sil"
        rnd*               ordinary pairs: a reference with a few edits
    files/lab/*.lab, files/rec/*.rec  four pairs as label files, for the run without a master label file (-L / default -X)
    norm.ref.mlf / norm.rec.mlf       names with contexts, mixed case and the label "x", for -s, -c and -e
The runs: default (label files), mlf (-I), f, t, p, n, nt (-n -t), z (-z sil -f -t -p), e (-e a x -f -t), c (-c -f -t), s (-s -f -t).
    python tests/golden/make_results_golden.py"""
import math
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "results")
WORDS = "abcde"

RUNS = {
    "default": (["-L", "files/lab"], ["files/rec/u1.rec", "files/rec/u2.rec", "files/rec/u3.rec", "files/rec/u4.rec"]),
    "mlf": (["-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "f": (["-f", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "t": (["-t", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "p": (["-p", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "n": (["-n", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "nt": (["-n", "-t", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "z": (["-z", "sil", "-f", "-t", "-p", "-I", "corner.ref.mlf"], ["corner.rec.mlf"]),
    "e": (["-e", "a", "x", "-f", "-t", "-I", "norm.ref.mlf"], ["norm.rec.mlf"]),
    "c": (["-c", "-f", "-t", "-I", "norm.ref.mlf"], ["norm.rec.mlf"]),
    "s": (["-s", "-f", "-t", "-I", "norm.ref.mlf"], ["norm.rec.mlf"]),
}


def dir_tile():
    src = open(os.path.join(ROOT, "htk_amd", "csrc", "results.hip")).read()
    return int(re.search(r"#define\s+RES_DIR_TILE\s+(\d+)", src).group(1))


def words(rng, n):
    return [rng.choice(WORDS) for _ in range(n)]


def edit(rng, ref, p=0.2):
    out = []
    for w in ref:
        x = rng.random()
        if x < p / 3:
            continue
        out.append(rng.choice(WORDS) if x < 2 * p / 3 else w)
        if x > 1 - p / 3:
            out.append(rng.choice(WORDS))
    return out


def corner_pairs():
    rng = random.Random(20)
    n = int(math.isqrt(dir_tile())) + 6                       # n * n grid cells: more than the tile
    r64 = words(rng, 64)
    long_ref = words(rng, n)
    P = [("one_hit", ["a"], ["a"]), ("one_sub", ["a"], ["b"]), ("one_130", ["c"], edit(rng, words(rng, 130), 0.0)[:130]), ("r130_one", words(rng, 130), ["d"]),
         ("w63", r64[:63], edit(rng, r64)[:64]), ("w64", r64, (edit(rng, r64) + r64)[:64]), ("w65", r64 + ["e"], (edit(rng, r64) + r64)[:64]),
         ("w64r", r64, (edit(rng, r64) + r64)[:65]),
         ("long", long_ref, edit(rng, long_ref)),
         ("tie_short", ["a"] * 5, ["a"] * 3), ("tie_long", ["a"] * 3, ["a"] * 5), ("tie_subins", ["a", "b", "c"], ["a", "d", "e", "c"]),
         ("tie_subdel", ["a", "d", "e", "c"], ["a", "b", "c"]), ("tie_cross", ["a", "b"], ["b", "a"]), ("tie_rep", ["a", "b", "a", "b", "a"], ["b", "a", "b"]),
         ("nul_start", ["sil", "a", "b"], ["a", "b"]), ("nul_end", ["a", "b"], ["a", "b", "sil"]), ("nul_double", ["a", "sil", "sil", "b"], ["a", "c", "b"]),
         ("nul_face", ["sil", "a", "sil", "b", "sil"], ["sil", "a", "b", "sil"]), ("nul_sub", ["a", "sil", "b"], ["a", "sil", "c", "sil"]),
         ("nul_all", ["sil", "sil", "sil"], ["sil", "sil"]), ("nul_vs_words", ["sil", "sil"], ["a", "b"]), ("words_vs_nul", ["a", "b", "c"], ["sil"])]
    for k in range(6):
        ref = words(rng, rng.randint(3, 30))
        P.append(("rnd%d" % k, ref, edit(rng, ref, 0.35)))
    return P


def norm_pairs():
    return [("n1", ["l-a+r", "b", "x", "C", "sil-d+e"], ["a", "q-b+r", "a", "c", "d"]),
            ("n2", ["Alpha", "beta", "x", "a"], ["alpha", "BETA", "a", "x", "X"]),
            ("n3", ["a-b", "c+d", "x-x+x", "e"], ["b", "c", "a", "E", "e+f"])]


def write_mlf(path, ext, pairs, which):
    with open(path, "w") as f:
        f.write("#!MLF!#\n")
        for p in pairs:
            f.write('"*/%s.%s"\n' % (p[0], ext))
            f.write("".join(w + "\n" for w in p[which]))
            f.write(".\n")


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "HResults")
    if not os.path.exists(exe):
        sys.exit("oracle/_ref/HResults is not built")
    os.makedirs(os.path.join(OUT, "files", "lab"), exist_ok=True)
    os.makedirs(os.path.join(OUT, "files", "rec"), exist_ok=True)
    open(os.path.join(OUT, "list"), "w").write("".join(w + "\n" for w in list(WORDS) + ["sil", "x"]))
    cp = corner_pairs()
    write_mlf(os.path.join(OUT, "corner.ref.mlf"), "lab", cp, 1)
    write_mlf(os.path.join(OUT, "corner.rec.mlf"), "rec", cp, 2)
    nm = norm_pairs()
    write_mlf(os.path.join(OUT, "norm.ref.mlf"), "lab", nm, 1)
    write_mlf(os.path.join(OUT, "norm.rec.mlf"), "rec", nm, 2)
    rng = random.Random(7)
    for k in range(1, 5):
        ref = words(rng, 4 + 3 * k)
        hyp = ref if k == 2 else edit(rng, ref, 0.4)
        open(os.path.join(OUT, "files", "lab", "u%d.lab" % k), "w").write("".join("%d %d %s\n" % (i * 100000, (i + 1) * 100000, w) for i, w in enumerate(ref)))
        open(os.path.join(OUT, "files", "rec", "u%d.rec" % k), "w").write("".join("%d %d %s %.3f\n" % (i * 100000, (i + 1) * 100000, w, -50.0 - i) for i, w in enumerate(hyp)))
    for name, (sw, hyp) in RUNS.items():
        r = subprocess.run([exe] + sw + ["list"] + hyp, cwd=OUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit("HResults %s failed:\n%s" % (name, r.stderr))
        open(os.path.join(OUT, name + ".out"), "w").write(r.stdout)
        print("%-8s %s" % (name, [l for l in r.stdout.splitlines() if l.startswith("WORD")]))


if __name__ == "__main__":
    main()
