"""The host side of lattice rescoring, without a device: the SLF reader, the visiting orders, the label lists, LatPrune's compaction and the
lattice writer against the reference's recorded files (tests/golden/latrescore, made by tests/golden/make_latrescore_golden.py), with the
numbers of the three recursions supplied by the plain restatement in latrescore_util.py -- which this pins to the reference for ALL fixtures,
so that the GPU tests may lean on it."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latrescore_util as lu

ROOT = lu.ROOT
RUNS = lu.fixtures()["runs"]


@pytest.fixture(scope="module")
def groups(native, tmp_path_factory):
    """Per group: the set read by the library, the lattices as the restatement reads them, its orders."""
    out = {}
    for g in lu.fixtures()["groups"]:
        d = str(tmp_path_factory.mktemp("lat_" + g))
        dpath, lats = lu.unpack_group(g, d)
        names = sorted(lats)
        ls = native.LatSet(dpath, "!SENT_START", "!SENT_END")
        for n in names:
            ls.add_file(lats[n])
        py = [lu.read_slf(lats[n]) for n in names]
        out[g] = dict(set=ls, names=names, lats=py, orders=[lu.orders(l) for l in py], dict=lu.read_dict(dpath), paths=lats, dict_path=dpath)
    return out


def beam(args, sw):
    if sw not in args:
        return None
    i = args.index(sw)
    return float(args[i + 1]), float(args[i + 2]) if i + 2 < len(args) and "." in args[i + 2] and args[i + 2][0].isdigit() else 0.0


def restated_run(native, G, run, tmp):
    """ProcessLattice (HLRescore.c:491) with latrescore_util's numbers and the library's host functions; returns {file name: text}, totals."""
    args, st = run["args"], lu.setting_of(run["args"])
    os.makedirs(os.path.join(tmp, "out"), exist_ok=True)
    cur, lats, ords = G["set"], list(G["lats"]), list(G["orders"])
    totals = {}

    def pruned(cur, lats, ords, b):
        dst = native.LatSet(like=cur)
        nl = []
        for u, (l, o) in enumerate(zip(lats, ords)):
            kn, ka = lu.prune(l, o, st, b[0], b[1])
            dst.add_pruned(cur, u, kn, ka)
            nl.append(lu.compact(l, kn, ka))
        return dst, nl, [lu.orders(l) for l in nl]

    if "-t" in args:
        cur, lats, ords = pruned(cur, lats, ords, beam(args, "-t"))
    if "-f" in args:
        mlf = native.MlfOut(os.path.join(tmp, "out.mlf")) if "-i" in args else None
        for u, n in enumerate(G["names"]):
            path, tot = lu.find_best(lats[u], ords[u], st)
            totals[n] = ["%.3f" % x for x in tot]
            tr = cur.trans(u, st, path)
            if "-o" in args:
                tr.format(frame_dur=1.0e7, flags=args[args.index("-o") + 1])
            if mlf:
                mlf.add("in/%s.rec" % n, tr)
            else:
                tr.write(os.path.join(tmp, "out", n + ".rec"))
        if mlf:
            mlf.close()
    if "-u" in args:
        cur, lats, ords = pruned(cur, lats, ords, beam(args, "-u"))
    if "-w" in args:
        for u, n in enumerate(G["names"]):
            score = None
            if run["sort"]:
                fw, bw, _ = lu.fb_max(lats[u], ords[u], st)
                score = fw + bw
            cur.write(u, st, os.path.join(tmp, "out", n + ".lat"), node_score=score)
    files = {}
    for f in sorted(os.listdir(os.path.join(tmp, "out"))):
        files["out/" + f] = open(os.path.join(tmp, "out", f)).read()
    if os.path.exists(os.path.join(tmp, "out.mlf")):
        files["out.mlf"] = open(os.path.join(tmp, "out.mlf")).read()
    return files, totals


def test_the_reader_reads_every_fixture_lattice(groups):
    n = 0
    for g in groups.values():
        assert len(g["set"]) == len(g["names"])
        for u, l in enumerate(g["lats"]):
            v = g["set"].view(u)
            assert (v["nNodes"], v["nArcs"]) == (l["nNodes"], l["nArcs"])
            for f in ("arcStart", "arcEnd", "arcAc", "arcLm", "arcPr", "nullEnd"):
                assert np.array_equal(v[f], l[f]), f
            assert np.array_equal(v["nodeTime"], l["nodeTime"])
            assert [g["set"].word_name(w) for w in v["nodeWord"]] == l["word"] and list(v["nodeVar"]) == l["var"]
            n += 1
    assert n >= 20


def test_the_visiting_orders_are_the_restatements(groups):
    for g in groups.values():
        for u, o in enumerate(g["orders"]):
            v = g["set"].view(u)
            assert (v["start"], v["end"]) == (o["start"], o["end"])
            assert np.array_equal(v["topOrder"], o["top"]) and np.array_equal(v["fwdArcs"], o["fwd"]) and np.array_equal(v["bwdArcs"], o["bwd"])
            assert o["top"][0] == o["start"]


@pytest.mark.parametrize("g", sorted(lu.fixtures()["groups"]))
def test_read_then_write_unsorted_is_the_references_file(groups, g, tmp_path):
    """-w with SORTLATTICE = F: node scores are zero, nothing is computed."""
    runs = [r for r in RUNS if r["group"] == g and r["name"] == "w_unsorted"]
    if g == "big":
        assert not runs
        return
    (run,) = runs
    G = groups[g]
    for u, n in enumerate(G["names"]):
        p = str(tmp_path / (n + ".lat"))
        G["set"].write(u, lu.setting_of(run["args"]), p)
        assert open(p).read() == run["files"]["out/%s.lat" % n], n


@pytest.mark.parametrize("rid", [r["id"] for r in RUNS])
def test_the_restatement_reproduces_the_reference(native, groups, rid, tmp_path):
    """Best paths (as label files), -T totals, pruned and sorted lattices of every fixture run, byte for byte."""
    run = next(r for r in RUNS if r["id"] == rid)
    files, totals = restated_run(native, groups[run["group"]], run, str(tmp_path))
    assert sorted(files) == sorted(run["files"])
    for f in run["files"]:
        assert files[f] == run["files"][f], f
    assert totals == run["totals"]


def test_the_fixtures_hold_what_they_were_built_for(groups):
    """Ties that the orders decide, both sides of the tile, the histogram branch and a tight beam that leaves one path."""
    tile = lu.fixtures()["tile"]
    sizes = {n: l["nNodes"] for n, l in zip(groups["random"]["names"], groups["random"]["lats"])}
    assert sizes["tile63"] == tile - 1 and sizes["tile64"] == tile and sizes["tile65"] == tile + 1 and sizes["one"] == 2
    assert groups["big"]["lats"][0]["nArcs"] >= 2900
    G = groups["random"]
    tied = 0
    for l, o in zip(G["lats"], G["orders"]):
        ka = lu.prune(l, o, (1, 5, -10.5, 1), 0.0)[1]             # a beam of nothing keeps the best route and whatever equals it
        tied += ka.sum() > len(lu.find_best(l, o, (1, 5, -10.5, 1))[0])
    assert tied >= 3
    st = (1.0, 2.0, 0.0, 0.0)
    narrowed = 0
    for l, o in zip(G["lats"] + groups["big"]["lats"], G["orders"] + groups["big"]["orders"]):
        a = lu.prune(l, o, st, 150.0, 40.0)[1].sum()
        b = lu.prune(l, o, st, 150.0, 0.0)[1].sum()
        narrowed += a < b
        kn, ka = lu.prune(l, o, (1, 5, -10.5, 1), 0.001)
        path, _ = lu.find_best(l, o, (1, 5, -10.5, 1))
        assert set(path) <= set(np.flatnonzero(ka))
    assert narrowed >= 2


def test_words_on_the_arcs(native, groups, tmp_path):
    """A lattice without node lines, its words on the arcs: each arc's word and variant go to its end node; a node line that comes after
    the arcs and names a word takes the lattice out of that form from there on, as ReadOneLattice's running format flag does."""
    G = groups["random"]
    ls = native.LatSet(like=G["set"])
    p = str(tmp_path / "alabs.lat")
    open(p, "w").write("VERSION=1.0\nN=4 L=4\nJ=0 S=0 E=1 W=W1 v=2 a=-10.0\nJ=1 S=0 E=2 W=NOV a=-11.0\nJ=2 S=1 E=3 W=!SENT_END a=-1.0\nJ=3 S=2 E=3 W=!SENT_END a=-1.0\n")
    u = ls.add_file(p)
    v = ls.view(u)
    assert [ls.word_name(w) for w in v["nodeWord"]] == ["!NULL", "W1", "NOV", "!SENT_END"] and list(v["nodeVar"]) == [-1, 2, -1, -1]
    open(p, "w").write("N=3 L=2\nJ=0 S=0 E=1 W=W1\nI=0 W=!NULL\nI=1 W=W1\nI=2 t=0.5 W=W2\nJ=1 S=1 E=2\n")
    v = ls.view(ls.add_file(p))
    assert [ls.word_name(w) for w in v["nodeWord"]] == ["!NULL", "W1", "W2"]
    out = str(tmp_path / "o.lat")
    ls.write(u, (1, 1, 0, 1), out, fmt="tvalr")
    assert "d=" not in open(out).read() and "W=NOV" in open(out).read()


def test_alignment_records_follow_the_format_letters(native, groups, tmp_path):
    """-q: d writes the records' labels, m their durations, n their likelihoods (OutputAlign HNet.c:503); the default has all three."""
    G = groups["nbx_wint_n3_t2500m"]
    ref = next(r for r in RUNS if r["id"] == "nbx_wint_n3_t2500m/w_unsorted")["files"]["out/u0.lat"]
    rec = [ln.split("d=")[1].strip() for ln in ref.splitlines() if "d=" in ln]
    assert rec
    u = G["names"].index("u0")
    for fmt, cut in (("tvalrd", lambda x: x.split(",")[0]), ("tvalrdm", lambda x: ",".join(x.split(",")[:2])), ("tvalrdmn", lambda x: x), ("tvalr", None)):
        p = str(tmp_path / (fmt + ".lat"))
        G["set"].write(u, (1.0, 5.0, -10.5, 1.0), p, fmt=fmt)
        got = [ln.split("d=")[1].strip() for ln in open(p).read().splitlines() if "d=" in ln]
        want = [] if cut is None else [":" + ":".join(cut(x) for x in r.strip(":").split(":")) + ":" for r in rec]
        assert got == want, fmt


def test_refusals(native, groups, tmp_path):
    G = groups["random"]
    src = open(G["paths"]["r12"]).read()

    def refused(text, what):
        p = str(tmp_path / "bad.lat")
        open(p, "w").write(text)
        with pytest.raises(native.HtkAmdError) as e:
            G["set"].add_file(p)
        assert what in str(e.value), str(e.value)

    n = len(G["set"])
    refused(src.replace("W=W3", "W=NOSUCH", 1) if "W=W3" in src else src.replace("W=!SENT_END", "W=NOSUCH"), "not in dict (8251)")
    refused(src[:len(src) // 2].rsplit("\n", 1)[0] + "\n", "Arcs unseen")
    refused("VERSION=1.0\n", "Premature end of lattice file before header")
    refused("VERSION=1.0\nSUBLAT=x\nN=2 L=1\nI=0 W=!NULL\nI=1 W=W1\nJ=0 S=0 E=1\n.\n", "sub-lattices")
    cyc = "N=4 L=4\nI=0 W=!NULL\nI=1 W=W1\nI=2 W=W2\nI=3 W=!NULL\nJ=0 S=0 E=1 a=-1.0\nJ=1 S=1 E=2 a=-1.0\nJ=2 S=2 E=1 a=-1.0\nJ=3 S=2 E=3 a=-1.0\n"
    refused(cyc, "Lattice contains cycles")
    refused("N=3 L=2\nI=0 W=!NULL\nI=1 W=W1\nI=2 W=W2\nJ=0 S=0 E=1\nJ=1 S=0 E=2\n", "Start/End nodes incorrect")
    refused("N=2 L=1\nI=0 W=!NULL\nI=1 W=W1\nJ=0 S=0 E=5\n", "does not contain end node 5")
    refused("N=99999999999 L=1\nJ=0 S=0 E=1 W=W1\n", "out of range")
    refused(src.replace(" r=", " d=:w1,x:w2: r=", 1), "ReadAlign: Cannot read duration 0")
    # words on the arcs (HLAT_ALABS, HNet.c:972 / :1078 / :1170-1182): the lattice carries them there as long as no node line has named a
    # word other than !NULL; an arc then NEEDS its W=, also where every node is !NULL (the reference says the same, 8250)
    refused("N=3 L=2\nJ=0 S=0 E=1\nJ=1 S=1 E=2 W=W2\n", "Need to know S,E [and W] for arc 0")
    refused("N=3 L=2\nI=0 W=!NULL\nI=1 W=!NULL\nI=2 W=!NULL\nJ=0 S=0 E=1 W=W1\nJ=1 S=1 E=2\n", "Need to know S,E [and W] for arc 1")
    assert len(G["set"]) == n
    with pytest.raises(native.HtkAmdError) as e:
        native.LatSet(G["dict_path"], "!NOT_THERE", "!SENT_END")
    assert "cannot find STARTWORD" in str(e.value)
    for sw in ("-n", "-m", "-c", "-I", "-d", "-P", "FIXBADLATS"):
        with pytest.raises(native.HtkAmdError) as e:
            native.latset_check_switch(sw)
        assert sw in str(e.value) and "not supported" in str(e.value)
    for sw in ("-f", "-t", "-u", "-w", "-s", "-p", "-a", "-r", "-i", "-l", "-y", "-o", "-L", "-X", "-q", "-C", "-T"):
        native.latset_check_switch(sw)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hlrescore_batch
    for argv in (["-f", "-n", "lm", "dict", "a.lat"], ["-f", "-I", "x.mlf", "dict", "a.lat"], ["-m", "f", "-w", "dict", "a.lat"]):
        with pytest.raises(native.HtkAmdError) as e:
            hlrescore_batch.main(argv)
        assert argv[1 if argv[0] == "-f" else 0] in str(e.value)


DRIVER = r"""
#include <stdio.h>
#include <string.h>
#include "htk_amd.h"
/* argv: dictionary, lattices, '!' + a file to write to; a lattice whose name starts with '!' must be REFUSED.  Reads, looks at the orders, writes, prunes to itself. */
int main(int argc, char **argv)
{
   htkamd_latset *s, *t;
   htkamd_lat_scales sc = {1.0f, 5.0f, -10.5f, 1.0f};
   static unsigned char keep[1 << 16];
   memset(keep, 1, sizeof(keep));
   if (htkamd_latset_create(argv[1], "!SENT_START", "!SENT_END", &s) || htkamd_latset_create_like(s, &t)) { printf("create: %s\n", htkamd_last_error()); return 2; }
   for (int i = 2; i < argc - 1; i++) {
      const int bad = argv[i][0] == '!';
      const int u = htkamd_latset_add_file(s, argv[i] + bad);
      if ((u < 0) != bad) { printf("%s: %d %s\n", argv[i], u, htkamd_last_error()); return 3; }
      if (u < 0) continue;
      htkamd_latset_view v;
      htkamd_trans *tr;
      if (htkamd_latset_get(s, u, &v) || v.nArcs > (1 << 16)) { printf("get: %s\n", htkamd_last_error()); return 4; }
      if (htkamd_latset_trans(s, u, &sc, v.fwdArcs, v.nArcs, &tr)) { printf("trans: %s\n", htkamd_last_error()); return 5; }
      htkamd_trans_free(tr);
      if (htkamd_latset_write(s, u, &sc, NULL, argv[argc - 1] + 1, 0)) { printf("write: %s\n", htkamd_last_error()); return 6; }
      if (htkamd_latset_add_pruned(t, s, u, keep, keep) != u) { printf("pruned: %s\n", htkamd_last_error()); return 7; }
   }
   printf("%d read\n", htkamd_latset_count(s));
   htkamd_latset_destroy(t); htkamd_latset_destroy(s);
   return 0;
}
"""


def test_the_host_code_is_clean_under_the_sanitizers(groups, tmp_path):
    """host/latrescore.c with a main of its own, built with -fsanitize=address,undefined and run as a child process over every fixture
    lattice and a handful of malformed ones."""
    host = os.path.join(ROOT, "htk_amd", "host")
    main_c = tmp_path / "drv.c"
    main_c.write_text(DRIVER + """
#include <stdarg.h>
static char err[4096];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof(err), fmt, ap); va_end(ap); }
const char *htkamd_last_error(void) { return err; }
const char *htkamd_net_word_name(const htkamd_net *n, int k) { (void)n; (void)k; return NULL; }
int htkamd_net_pron_num(const htkamd_net *n, int k) { (void)n; (void)k; return 0; }
int htkamd_results_label_id(htkamd_results *r, const char *name) { (void)r; (void)name; return 0; }
""")
    exe = str(tmp_path / "drv")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           str(main_c), os.path.join(host, "latrescore.c"), os.path.join(host, "slfout.c"), os.path.join(host, "labio.c"), os.path.join(host, "htktext.c"), "-o", exe, "-lm"])
    bad = []
    good = open(groups["random"]["paths"]["r20"]).read()
    for i, text in enumerate(["", "N=2", "N=2 L=1\nI=0 W=\n", "N=2 L=1\nI=7\n", "N=2 L=1\nJ=0 S=0\n", good[:len(good) // 3], good.replace(" S=", " S~", 1),
                              good.replace(" E=", " E=9999", 1), "N=1000000 L=1\nJ=0 S=0 E=999999\n", "N=2 L=1\nI=0 W=\"unterminated\nJ=0 S=0 E=1\n",
                              "N=3 L=3\nJ=0 S=0 E=1\nJ=1 S=1 E=0\nJ=2 S=1 E=2\n", "N=-5 L=-5\n\n", "N=99999999999 L=1\nJ=0 S=0 E=1\n",
                              good.replace(" r=", " d=:a,x: r=", 1), good.replace(" r=", " d=:a,0.1,-3.0,b: r=", 1)]):
        p = tmp_path / ("bad%d.lat" % i)
        p.write_text(text)
        bad.append("!" + str(p))
    for g in groups.values():
        argv = [exe, g["dict_path"]] + [g["paths"][n] for n in g["names"]] + bad + ["!" + str(tmp_path / "scratch.lat")]
        p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        assert "%d read" % len(g["names"]) in p.stdout
