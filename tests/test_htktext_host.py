"""The host text layer (htk_amd/host/htktext.c) against the reference's own answers, recorded in tests/golden/htktext/htktext.json by
tests/golden/make_htktext_golden.py: ReadString token by token, ReWriteString under each quote argument, label files through
htkamd_labels_read, dictionaries through the shared dictionary reader.  htktext.c and labio.c are built with a main of their own under
-fsanitize=address,undefined and run as a child process; nothing is loaded into Python."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "htktext", "htktext.json")))

DRIVER = r"""
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "htk_amd.h"
#include "htktext.h"
static char err[4096];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof(err), fmt, ap); va_end(ap); }
static void hex(const char *s) { if (!*s) printf("''"); for (; *s; s++) printf("%02x", (unsigned char)*s); }
static int fail(const char *what) { fprintf(stderr, "%s: %s\n", what, err); return 1; }
int main(int argc, char **argv)
{
   static char buf[1024], in[1024], out[4200];
   const char *mode = argv[1], *arg = argv[2];
   if (argc != 3) return 2;
   if (!strcmp(mode, "write") || !strcmp(mode, "roundtrip")) {
      static const char quotes[4] = {0, '\'', '"', '\\'};
      size_t n = strlen(arg) / 2, i;
      for (i = 0; i < n; i++) { unsigned v; sscanf(arg + 2 * i, "%2x", &v); in[i] = (char)v; }
      in[n] = 0;
      for (int k = 0; k < 4; k++) {
         const size_t L = htx_rewrite(in, quotes[k], out, sizeof(out));
         if (L >= sizeof(out) || L != strlen(out)) { snprintf(err, sizeof(err), "length %zu", L); return fail("rewrite"); }
         char tiny[4]; if (htx_rewrite(in, quotes[k], tiny, sizeof(tiny)) != L || strlen(tiny) > 3) return fail("rewrite bound");
         if (mode[0] == 'w') { hex(out); printf("\n"); continue; }
         htx_src s = {out, out + L, 0};
         const int r = htx_read_string(&s, 0, NULL, buf, sizeof(buf));
         printf("%d\n", (n == 0 && r == HTX_NONE && !quotes[k]) || (r == HTX_GOT && s.p == s.end && !strcmp(buf, in)));
      }
      return 0;
   }
   if (!strcmp(mode, "labels")) {
      htkamd_labels *L;
      if (htkamd_labels_read(arg, &L)) return fail("labels_read");
      for (int i = 0; i < htkamd_labels_count(L); i++) {
         hex(htkamd_labels_name(L, i)); printf(" %.9g %lld %lld\n", htkamd_labels_score(L, i), htkamd_labels_start(L, i), htkamd_labels_end(L, i));
      }
      htkamd_labels_free(L);
      return 0;
   }
   if (!strcmp(mode, "mlf")) {
      htkamd_mlf *m;
      if (htkamd_mlf_read(arg, &m)) return fail("mlf_read");
      for (int i = 0; i < htkamd_mlf_count(m); i++) {
         const htkamd_labels *L = htkamd_mlf_entry(m, i);
         hex(htkamd_mlf_pattern(m, i)); printf("\n");
         for (int k = 0; k < htkamd_labels_count(L); k++) { printf(" "); hex(htkamd_labels_name(L, k)); printf(" %.9g\n", htkamd_labels_score(L, k)); }
      }
      htkamd_mlf_free(m);
      return 0;
   }
   size_t len; int why;
   char *txt = htx_read_file(arg, &len, &why);
   if (!txt) { snprintf(err, sizeof(err), "%s", why == HTX_EOPEN ? "cannot open" : "out of memory"); return fail("read_file"); }
   if (strlen(txt) > len || txt[len]) return 3;
   htx_src s = {txt, txt + len, 0};
   int rc = 0;
   if (!strcmp(mode, "read") || !strcmp(mode, "alpha3") || !strcmp(mode, "alpha4")) {
      const char *stops = mode[0] == 'r' ? NULL : (mode[5] == '3' ? ".,)" : ".,)}");
      for (;;) {
         const int r = htx_read_string(&s, 0, stops, buf, sizeof(buf));
         if (r == HTX_GOT) { printf("T "); hex(buf); printf(" %d\n", s.wasQuoted); if (stops && s.p < s.end && strchr(stops, *s.p)) printf("S %c\n", *s.p++); continue; }
         if (r < 0) { snprintf(err, sizeof(err), "%s", htx_result_text(r)); fflush(stdout); rc = fail("read_string"); break; }
         printf("F\n");
         if (s.p >= s.end) break;
      }
   } else if (!strcmp(mode, "dict")) {
      htx_dict_entry e = {0};
      char **seen = NULL; int nSeen = 0, r;
      while ((r = htx_dict_next(&s, arg, &e)) == HTX_GOT) {
         int pnum = 1;
         for (int i = 0; i < nSeen; i++) pnum += !strcmp(seen[i], e.word);
         seen = (char **)realloc(seen, sizeof(char *) * (size_t)(nSeen + 1)); seen[nSeen++] = strdup(e.word);
         hex(e.word); printf(" %d ", pnum);
         if (e.outKind == HTX_OUT_EMPTY) printf("-"); else hex(e.outKind == HTX_OUT_GIVEN ? e.outSym : e.word);
         printf(" %.9g", !e.hasProb ? 0.0 : (e.prob >= 1.0E-6f ? (float)log((double)e.prob) : -1.0E10f));      /* NewPron HDict.c:144 */
         for (int k = 0; k < e.nPhones; k++) { printf(" "); hex(e.phone[k]); }
         printf("\n");
      }
      for (int i = 0; i < nSeen; i++) free(seen[i]);
      free(seen); htx_dict_free(&e);
      if (r) rc = fail("dict");
   } else rc = 2;
   free(txt);
   return rc;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("htktext")
    host = os.path.join(ROOT, "htk_amd", "host")
    (d / "drv.c").write_text(DRIVER)
    out = str(d / "drv")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           "-I" + host, str(d / "drv.c"), os.path.join(host, "htktext.c"), os.path.join(host, "labio.c"), "-o", out, "-lm"])

    def run(mode, data, as_file=True):
        arg = data.hex()
        if as_file:
            p = d / "in.txt"
            p.write_bytes(data)
            arg = str(p)
        r = subprocess.run([out, mode, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode in (0, 1), r.stderr[-3000:]                      # 1: a refusal with a message; anything else: the sanitizers or a crash
        assert r.returncode == 0 or r.stderr.strip().split(": ", 1)[1], r.stderr
        return r.returncode == 0, r.stdout.splitlines(), r.stderr
    return run


def test_read_string_reads_what_the_reference_reads(exe):
    """Token by token, the wasQuoted flag included; where the reference refuses (an open quote, more than its 1023 characters), so does
    the shared reader, after the same tokens."""
    for rec in GOLD["read"]:
        ok, out, _ = exe("read", bytes.fromhex(rec["in"]))
        assert (ok, out) == (rec["ok"], rec["out"]), bytes.fromhex(rec["in"])[:60]


def test_stop_sets_end_a_bare_string_only(exe):
    """ParseAlpha's ".,)" and GetAlpha's ".,)}": each stop character ends an unquoted string and is left unread; inside quotes it is text."""
    for mode, stops in (("alpha3", ".,)"), ("alpha4", ".,)}")):
        for c in ".,)}":
            ok, out, _ = exe(mode, ("a%cb 'a%cb'\n" % (c, c)).encode())
            quoted = "T %s 1" % ("a%cb" % c).encode().hex()
            bare = ["T 61 0", "S " + c, "T 62 0"] if c in stops else ["T %s 0" % ("a%cb" % c).encode().hex()]
            assert ok and out == bare + [quoted, "F"], (mode, c, out)


def test_rewrite_writes_what_the_reference_writes(exe):
    for rec in GOLD["write"]:
        ok, out, _ = exe("write", bytes.fromhex(rec["in"]), as_file=False)
        assert ok and out == rec["out"], bytes.fromhex(rec["in"])


def test_what_is_written_reads_back(exe):
    """Every recorded string, written under either quote character, reads back as its own bytes; so it does unquoted (q = 0 and the
    escape character) unless it holds white space, which the reference's unquoted forms leave bare too."""
    strings = {r["in"] for r in GOLD["write"]}
    for rec in GOLD["read"]:
        strings |= {t.split()[1] for t in rec["out"] if t.startswith("T ") and t.split()[1] != "''"}
    assert len(strings) > 30
    for h in sorted(strings):
        raw = bytes.fromhex(h)
        ok, out, _ = exe("roundtrip", raw, as_file=False)
        assert ok and out[1] == "1" and out[2] == "1", raw
        if not any(c in raw for c in b" \t\n\r\v\f"):
            assert out[0] == "1" and out[3] == "1", raw


def test_labels_read_names_and_scores_as_the_reference(exe):
    for rec in GOLD["labels"]:
        ok, out, err = exe("labels", bytes.fromhex(rec["in"]))
        assert ok == rec["ok"], err
        if ok:
            assert [l.split() for l in out] == [l.split() for l in rec["out"]]
    # the same names through a master label file, whose pattern is a ReadString string too
    ok, out, err = exe("mlf", b'#!MLF!#\n"*/a\\"b.lab"\n' + bytes.fromhex(GOLD["labels"][0]["in"]) + b".\n")
    assert ok, err
    assert out[0] == b'*/a"b.lab'.hex() and [l.split()[0] for l in out[1:]] == [l.split()[0] for l in GOLD["labels"][0]["out"]]


def test_dictionary_entries_as_the_reference(exe):
    """The reference hashes its words, so the entries are compared as sets of lines.  A refusal of the reference is a refusal here."""
    for rec in GOLD["dict"]:
        ok, out, err = exe("dict", bytes.fromhex(rec["in"]))
        assert ok == rec["ok"], (bytes.fromhex(rec["in"])[:40], err)
        if ok:
            assert sorted(out) == sorted(rec["out"]), bytes.fromhex(rec["in"])[:40]


def test_malformed_input_is_refused_with_a_message(exe):
    long_name = b"0 100 " + b"n" * (1 << 20)                      # one long line, no newline
    for mode, data in (("read", b'"open'), ("read", b"x" * 5000), ("labels", b'0 1 "open\n'), ("labels", b"0 1 'open"), ("labels", long_name),
                       ("mlf", b""), ("mlf", b'#!MLF!#\n"open\n'), ("mlf", b'#!MLF!#\n"*"\n' + long_name), ("dict", b'W "open\n'), ("dict", b"W 'open"),
                       ("dict", b"W [a] [b] p\n"), ("dict", b"W 7 p\n")):
        ok, _, err = exe(mode, data)
        assert not ok and len(err.strip()) > 10, (mode, data[:30])
    # not malformed: an empty file holds nothing; a dictionary that is one long line without a newline is one entry
    for mode in ("read", "labels", "dict"):
        ok, out, _ = exe(mode, b"")
        assert ok and out == (["F"] if mode == "read" else [])
    ok, out, _ = exe("dict", b"W " + b" ".join(b"p%d" % i for i in range(3000)))
    assert ok and len(out) == 1 and len(out[0].split()) == 4 + 3000


SLF_DRIVER = r"""
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "htk_amd.h"
static char err[4096];
void htkamd_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof(err), fmt, ap); va_end(ap); }
const char *htkamd_last_error(void) { return err; }
int htkamd_results_label_id(htkamd_results *r, const char *name) { (void)r; (void)name; return 0; }
static void hex(const char *s) { for (; *s; s++) printf("%02x", (unsigned char)*s); }
/* argv: MMF, HMM list, dictionary, SLF.  Prints the node words and the arcs (start word, end word, l=) as each reader saw them. */
int main(int argc, char **argv)
{
   htkamd_mmf *m; htkamd_net *net; htkamd_latset *ls; htkamd_latset_view v;
   if (argc != 5) return 2;
   if (htkamd_mmf_create(&m) || htkamd_mmf_read(m, argv[1], NULL) || htkamd_mmf_finish(m, argv[2], NULL, NULL)) { fprintf(stderr, "mmf: %s\n", err); return 1; }
   if (htkamd_net_build(argv[4], argv[3], m, &net)) { fprintf(stderr, "net_build: %s\n", err); return 1; }
   const htkamd_net_desc *d = htkamd_net_get(net);
   for (int n = 0; n < d->nNodes; n++) {
      if (d->kind[n] != HTKAMD_NODE_WORD) continue;
      printf("net node "); hex(htkamd_net_word_name(net, d->model[n])); printf("\n");
      for (int k = d->linkOff[n]; k < d->linkOff[n + 1]; k++) {
         int t = d->linkDest[k];                       /* down the chain of models to the word node of the arc's end */
         while (d->kind[t] == HTKAMD_NODE_HMM) t = d->linkDest[d->linkOff[t]];
         if (d->kind[t] != HTKAMD_NODE_WORD) continue; /* the network's final node */
         printf("net arc "); hex(htkamd_net_word_name(net, d->model[n])); printf(" "); hex(htkamd_net_word_name(net, d->model[t])); printf(" %g\n", d->linkLike[k]);
      }
   }
   if (htkamd_latset_create(argv[3], NULL, NULL, &ls)) { fprintf(stderr, "latset_create: %s\n", err); return 1; }
   const int u = htkamd_latset_add_file(ls, argv[4]);
   if (u < 0 || htkamd_latset_get(ls, u, &v)) { fprintf(stderr, "latset_add_file: %s\n", err); return 1; }
   for (int n = 0; n < v.nNodes; n++) { printf("lat node "); hex(htkamd_latset_word_name(ls, v.nodeWord[n])); printf("\n"); }
   for (int a = 0; a < v.nArcs; a++) {
      printf("lat arc "); hex(htkamd_latset_word_name(ls, v.nodeWord[v.arcStart[a]])); printf(" "); hex(htkamd_latset_word_name(ls, v.nodeWord[v.arcEnd[a]])); printf(" %g\n", v.arcLm[a]);
   }
   htkamd_latset_destroy(ls); htkamd_net_destroy(net); htkamd_mmf_destroy(m);
   return 0;
}
"""


def test_both_slf_readers_see_the_same_lattice(tmp_path):
    """One SLF with a single-quoted W= value, an escaped quote in a word and a J= line longer than 4096 bytes, read by the network
    builder (htkamd_net_build) and by the lattice set (htkamd_latset_add_file): the same node words and arc end points, and the right ones."""
    host = os.path.join(ROOT, "htk_amd", "host")
    fix = os.path.join(ROOT, "tests", "golden", "decode", "bigram")
    (tmp_path / "drv.c").write_text(SLF_DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), str(tmp_path / "drv.c")] +
                          [os.path.join(host, f) for f in ("net.c", "mmf.c", "prep.c", "cepsnorm.c", "accio.c", "latrescore.c", "slfout.c", "labio.c", "htktext.c")] + ["-o", exe, "-lm"])
    words = [b"two words", b'it"s', b"q'x", b"END"]
    (tmp_path / "dict").write_bytes(b"'two words' p0 p1\nit\\\"s p2\n\"q'x\" p3 p4\nEND p5\n")
    pad = b" ".join(b"x%d=%s" % (i, b"y" * 1000) for i in range(5))
    slf = (b"VERSION=1.0\nN=4 L=3\nI=0 W='two words'\nI=1 W=it\\\"s\nI=2 W=\"q'x\"\nI=3 W=END\n"
           b"J=0 S=0 E=1 l=-1.5\nJ=1 S=1 E=2 " + pad + b" l=-2.5\nJ=2 S=2 E=3 l=-0.5\n")
    assert max(len(l) for l in slf.split(b"\n")) > 4096
    (tmp_path / "a.slf").write_bytes(slf)
    r = subprocess.run([exe, os.path.join(fix, "MMF"), os.path.join(fix, "hmmlist"), str(tmp_path / "dict"), str(tmp_path / "a.slf")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {who: sorted(l[len(who) + 1:] for l in r.stdout.splitlines() if l.startswith(who + " ")) for who in ("net", "lat")}
    want = sorted(["node " + w.hex() for w in words] + ["arc %s %s %s" % (words[i].hex(), words[i + 1].hex(), l) for i, l in enumerate(("-1.5", "-2.5", "-0.5"))])
    assert seen["net"] == want and seen["lat"] == want, r.stdout
