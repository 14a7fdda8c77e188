"""Known answers for lattice rescoring: the reference's HLRescore (oracle/_ref/HLRescore, built by `make -C oracle _ref/HLRescore`) over
  (a) the committed lattices of tests/golden/decode/rescore/lat and of EVERY case under tests/golden/decode/nbest, each with its case's
      dictionary extended by the two boundary words (three cases under all switch sets, the others under those of SMALL_RUNS), and
  (b) seeded random DAG lattices written here (likelihoods with two decimals, as SLF carries them): one arc; parallel arcs and parallel
      two-arc routes of exactly equal total, so that the order of the lists decides the path; !NULL nodes inside; node numbers and J= lines
      not in time order; a word with a missing pronunciation variant; a word whose output symbol is empty; 63 / 64 / 65 nodes (both sides
      of htkamd_latset_tile() = 64); one of about 3 000 arcs,
under the switch sets of RUNS.  Writes tests/golden/latrescore/fixtures.json.gz: the inputs that are not committed elsewhere, every file
the reference wrote, and the `ac lm pr tot` line of LatFindBest's trace (HLAT: TRACE = 32) per file.  Data only.  Every run must exit 0.
Run from the repository root on a machine that has the reference:  python tests/golden/make_latrescore_golden.py"""
import gzip
import json
import os
import random
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "latrescore")
BIN = os.path.join(ROOT, "oracle", "_ref", "HLRescore")
TILE = 64
BOUNDARY = "!SENT_START []\n!SENT_END []\n"

RAND_DICT = "".join("W%d w%d\n" % (i, i) for i in range(8)) + "W1 [one] w1 x\nW2 0.4 w2 y\nW2 [two] 0.6 w2 z\nNOV n\nSIL [] sil\n" + BOUNDARY

# (name, switches, SORTLATTICE); -l out is added to all but the -i run
F5 = [("f_default", ["-f"]), ("f_s5_pm10", ["-f", "-s", "5.0", "-p", "-10.5"]), ("f_s0_p3_a05", ["-f", "-s", "0.0", "-p", "3.25", "-a", "0.5"]),
      ("f_s12_pm2_r25_a15", ["-f", "-s", "12.3", "-p", "-2.0", "-r", "2.5", "-a", "1.5"]), ("f_s2_r0", ["-f", "-s", "2.0", "-r", "0.0"])]
RUNS = [(n, a, True) for n, a in F5] + [
    ("f_mlf", ["-f", "-i", "out.mlf", "-s", "5.0", "-p", "-10.5"], True),
    ("f_s1_pm10", ["-f", "-p", "-10.5"], True),                   # with f_default, f_s5_pm10 and f_s5_p0: a 2 x 2 grid over -s and -p
    ("f_s5_p0", ["-f", "-s", "5.0"], True),
    ("f_oST", ["-f", "-o", "ST", "-s", "5.0", "-p", "-10.5"], True),
    ("t_tight", ["-t", "0.001", "-f", "-w", "-s", "5.0", "-p", "-10.5"], True),
    ("t_wide", ["-t", "9000.0", "-f", "-w"], True),
    ("t_aps", ["-t", "150.0", "40.0", "-f", "-w", "-s", "2.0", "-r", "0.0"], True),
    ("u_30", ["-f", "-u", "30.0", "-w", "-s", "5.0", "-p", "-10.5"], True),
    ("w_sorted", ["-w", "-s", "5.0", "-p", "-10.5"], True),
    ("w_unsorted", ["-w", "-s", "5.0", "-p", "-10.5"], False),
]
SMALL_RUNS = {"f_default", "f_s5_pm10", "t_aps", "u_30", "w_sorted", "w_unsorted"}      # the N-best cases beyond the first three: size
BIG_RUNS = {"f_default", "f_s5_pm10", "f_s0_p3_a05", "f_s12_pm2_r25_a15", "f_s2_r0", "t_aps", "t_tight"}      # the 3 000-arc lattice: where size matters


def random_lattice(rng, nn, na, name, special=False):
    """Nodes 0 .. nn-1 in time order, then renumbered at random; every node lies on a route from the first to the last."""
    arcs = set()
    for i in range(1, nn):
        arcs.add((rng.randrange(max(0, i - 6), i), i))
    for i in range(nn - 1):
        arcs.add((i, rng.randrange(i + 1, min(nn, i + 7))))
    while len(arcs) < na - (6 if special else 0) and len(arcs) < nn * (nn - 1) // 2:
        i = rng.randrange(nn - 1)
        arcs.add((i, rng.randrange(i + 1, min(nn, i + 9))))
    words = ["!NULL"] + [("W%d" % rng.randrange(8), 1) for _ in range(nn - 2)] + [("!SENT_END", 1)]
    words[0] = ("!NULL", -1)
    for i in range(1, nn - 1):
        r = rng.random()
        if words[i][0] == "W2" or words[i][0] == "W1":
            words[i] = (words[i][0], rng.choice([1, 2]))
        if r < 0.08:
            words[i] = ("!NULL", -1)
        elif r < 0.14:
            words[i] = ("NOV", 3)                              # no such variant: the word's name is the label
        elif r < 0.20:
            words[i] = ("SIL", 1)                              # empty output symbol: no label
    rec = []
    for s, e in sorted(arcs):
        rec.append([s, e, -round(rng.uniform(40, 300), 2), -round(rng.uniform(0, 8), 2), rng.choice([0.0, -0.36, -0.92, -1.2])])
    times = [n * 0.03 for n in range(nn)]
    if special and nn >= 8:
        # m: the middle of the best route under -s 5 -p -10.5 (a plain fp64 pass is near enough to choose it), so that the ties decide the answer
        sc, bk = [0.0] + [-1e30] * (nn - 1), [None] * nn
        for s2, e2, a2, l2, r2 in sorted(rec):
            v = sc[s2] + a2 + 5.0 * l2 + r2 - 10.5
            if v > sc[e2]:
                sc[e2], bk[e2] = v, s2
        route = [nn - 1]
        while bk[route[-1]] is not None:
            route.append(bk[route[-1]])
        m = route[len(route) // 2]
        if m in (0, nn - 1):
            m = nn // 2
        s, e, a, l, r = next(x for x in rec if x[1] == m)
        rec.append([s, e, a, l, r]); rec.append([s, e, a, l, r])       # parallel arcs of equal total
        # a twin of node m -- same word, same time, the same arcs with the same numbers: routes of equal total through m and its twin
        words.append(words[m]); times.append(times[m])
        rec += [[s2, nn, a2, l2, r2] for s2, e2, a2, l2, r2 in rec if e2 == m] + [[nn, e2, a2, l2, r2] for s2, e2, a2, l2, r2 in rec if s2 == m]
        nn += 1
    perm = list(range(nn)); rng.shuffle(perm)
    ids = list(range(len(rec))); rng.shuffle(ids)                # J numbers differ from the order of the lines
    lines = ["VERSION=1.0", "UTTERANCE=%s.mfc" % name, "lmname=net.slf", "lmscale=1.00   wdpenalty=0.00  ", "acscale=1.00  ", "vocab=dict", "N=%-4d L=%-5d" % (nn, len(rec))]
    for n in sorted(range(nn), key=lambda i: perm[i]):
        w, v = words[n]
        lines.append("I=%-4d t=%-5.2f W=%-19s %s" % (perm[n], times[n], w, "v=%-2d " % v if v >= 0 else ""))
    order = list(range(len(rec))); rng.shuffle(order)
    for k in order:
        s, e, a, l, r = rec[k]
        lines.append("J=%-5d S=%-4d E=%-4d a=%-9.2f l=%-7.3f r=%-6.2f " % (ids[k], perm[s], perm[e], a, l, r))
    return "\n".join(lines) + "\n"


def groups():
    g = {}
    full = {"bigram_n4_t2500": "nb_bigram", "tee_n3_t2500": "nb_tee", "loop_n3_t2500": "nb_loop"}
    cases = [("rescore", "tests/golden/decode/rescore/lat", "bigram")]
    for d in sorted(os.listdir(os.path.join(ROOT, "tests/golden/decode/nbest"))):
        if os.path.isdir(os.path.join(ROOT, "tests/golden/decode/nbest", d)):
            case = json.load(open(os.path.join(ROOT, "tests/golden/decode/nbest", d, "nbest.json")))["case"]
            cases.append((full.get(d, "nbx_" + d), "tests/golden/decode/nbest/" + d, case))
    for name, src, case in cases:
        lats = {f[:-4]: dict(path=src + "/" + f) for f in sorted(os.listdir(os.path.join(ROOT, src))) if f.endswith(".lat")}
        g[name] = dict(dict=open(os.path.join(ROOT, "tests/golden/decode", case, "dict")).read() + BOUNDARY, lats=lats)
    rng = random.Random(20240611)
    lats = {"one": "VERSION=1.0\nUTTERANCE=one.mfc\nlmname=net.slf\nN=2    L=1    \nI=0    t=0.00  W=!NULL\nI=1    t=0.31  W=W3 v=1\nJ=0     S=0    E=1    a=-123.45   l=-2.500  r=0.00\n"}
    for name, nn, na, sp in (("r12", 12, 30, True), ("r20", 20, 60, True), ("r31", 31, 70, False), ("tile63", TILE - 2, 150, True), ("tile64", TILE - 1, 160, True),
                             ("tile65", TILE, 170, True), ("r90", 90, 300, True)):
        lats[name] = random_lattice(rng, nn, na, name, sp)      # (a special lattice gains one twin node: 63, 64, 65 nodes)
    g["random"] = dict(dict=RAND_DICT, lats=lats)
    g["big"] = dict(dict=RAND_DICT, lats={"big3000": random_lattice(rng, 700, 3000, "big3000", True)})
    return g


def main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/HLRescore"])
    G = groups()
    runs = []
    for gname, g in G.items():
        for rname, args, sort in RUNS:
            if (gname == "big" and rname not in BIG_RUNS) or (gname.startswith("nbx_") and rname not in SMALL_RUNS):
                continue
            d = tempfile.mkdtemp()
            try:
                os.makedirs(os.path.join(d, "in")); os.makedirs(os.path.join(d, "out"))
                open(os.path.join(d, "dict"), "w").write(g["dict"])
                open(os.path.join(d, "cfg"), "w").write("STARTWORD = !SENT_START\nENDWORD = !SENT_END\nSORTLATTICE = %s\nHLAT: TRACE = 32\n" % ("T" if sort else "F"))
                for n, t in g["lats"].items():
                    if isinstance(t, dict):
                        shutil.copy(os.path.join(ROOT, t["path"]), os.path.join(d, "in", n + ".lat"))
                    else:
                        open(os.path.join(d, "in", n + ".lat"), "w").write(t)
                names = sorted(g["lats"])
                cmd = [BIN, "-C", "cfg"] + args + ([] if "-i" in args else ["-l", "out"]) + ["dict"] + ["in/%s.lat" % n for n in names]
                p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if p.returncode != 0:
                    sys.exit("%s / %s: HLRescore exited %d\n%s" % (gname, rname, p.returncode, p.stdout[-2000:]))
                tot = re.findall(r"^ac lm pr tot: (\S+) (\S+) (\S+) (\S+)$", p.stdout, re.M)
                if "-f" in args and len(tot) != len(names):
                    sys.exit("%s / %s: %d totals for %d lattices" % (gname, rname, len(tot), len(names)))
                files = {}
                for f in sorted(os.listdir(os.path.join(d, "out"))):
                    files["out/" + f] = open(os.path.join(d, "out", f)).read()
                if os.path.exists(os.path.join(d, "out.mlf")):
                    files["out.mlf"] = open(os.path.join(d, "out.mlf")).read()
                want = (len(names) if "-f" in args and "-i" not in args else 0) + (len(names) if "-w" in args else 0) + ("-i" in args)
                if len(files) != want:
                    sys.exit("%s / %s: %d files written, %d expected" % (gname, rname, len(files), want))
                runs.append(dict(id=gname + "/" + rname, group=gname, name=rname, args=args, sort=sort, lats=names, files=files,
                                 totals={n: list(t) for n, t in zip(names, tot)} if "-f" in args else {}))
            finally:
                shutil.rmtree(d)
    os.makedirs(OUT, exist_ok=True)
    blob = json.dumps(dict(tile=TILE, groups=G, runs=runs), sort_keys=True).encode()
    with open(os.path.join(OUT, "fixtures.json.gz"), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, compresslevel=9) as z:
            z.write(blob)
    print("%d runs, %d bytes" % (len(runs), os.path.getsize(os.path.join(OUT, "fixtures.json.gz"))))


if __name__ == "__main__":
    main()
