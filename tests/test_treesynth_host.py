"""Unseen triphones from the trees, the host side (htk_amd/host/treesynth.c): HHEd's LT with ST, CO, and the script front end, against
what the reference's HHEd wrote for the fixture (tests/golden/make_synth_golden.py).  AU's matching and tree walks run on the device:
tests/test_gpu_treesynth.py."""
import glob
import os
import re
import subprocess

import pytest

import treeclust_util as tu
import treesynth_util as su
from treeclust_util import G

EINVAL, EMODEL, EIO = -1, -5, -6
HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER><DIAGC>\n"
MAT = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n"


def state(mean):
    return "<MEAN> 2\n%s\n<VARIANCE> 2\n1 1\n" % mean


def hmm(name, st, tr):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s<ENDHMM>\n' % (name, st, tr)


def load(native, tmp_path, mmf_name, lst="seen"):
    w = su.workdir(tmp_path, mmf_name)
    return native.Mmf([os.path.join(w, "in.mmf")], hmm_list=os.path.join(w, lst)), w


def reverse_patterns(trees: bytes) -> bytes:
    """What one LT + ST does to a trees file, with HHEd as here: LoadQuestion prepends the patterns, ShowTrees writes the list."""
    def rev(m):
        return m.group(1) + b",".join(reversed(m.group(2).split(b","))) + m.group(3)
    return re.sub(rb"(?m)^(QS \S+ \{ )(.*)( \})$", rev, trees)


def hand_set(native, tmp_path):
    text = HDR + "".join('~s "%s"\n%s' % (n, state("%d 0" % k)) for k, n in enumerate(("ST_aa_2_1", "ST_aa_2_2", "ST_aa_2_3", "ST_sil_3_1")))
    text += hmm("aa", '~s "ST_aa_2_1"\n', MAT)
    (tmp_path / "hand.mmf").write_text(text)
    return native.Mmf(files=[str(tmp_path / "hand.mmf")])


@pytest.mark.parametrize("trees,mmf", [("trees1", "tied1.mmf"), ("trees2", "tied2.mmf"), ("trees3", "tied3.mmf"), ("trees_hand.expected", None)])
def test_lt_st_round_trip(native, tmp_path, trees, mmf):
    """LT + ST gives the file back with every question's patterns in the opposite order -- HHEd does the same (treesA.lt_st is its
    output) --, the trees themselves byte for byte; a second round gives the first file back byte for byte."""
    src = tu.golden_bytes(trees)
    if mmf:
        with open(tmp_path / "in.mmf", "wb") as f:
            f.write(tu.golden_bytes(mmf))
        _, lst = tu.unpack_inputs(tmp_path)
        m = native.Mmf([str(tmp_path / "in.mmf")], hmm_list=lst)
    else:
        m = hand_set(native, tmp_path)
    (tmp_path / "t0").write_bytes(src)
    m.load_trees(str(tmp_path / "t0")); m.save_trees(str(tmp_path / "t1"))
    once = (tmp_path / "t1").read_bytes()
    assert once == reverse_patterns(src)
    assert once.split(b"\n\n", 1)[1] == src.split(b"\n\n", 1)[1]                 # the trees: byte for byte
    if trees == "trees1":
        assert src == su.golden_bytes("treesA") and once == su.golden_bytes("treesA.lt_st")
    m2 = hand_set(native, tmp_path) if not mmf else native.Mmf([str(tmp_path / "in.mmf")], hmm_list=lst)
    m2.load_trees(str(tmp_path / "t1")); m2.save_trees(str(tmp_path / "t2"))
    assert (tmp_path / "t2").read_bytes() == src
    held = m.trees()
    assert [(t["name"], t["state"]) for t in held] == [(a.decode(), int(b)) for a, b in re.findall(rb"(?m)^(\w+)\[(\d)\]$", src)]


def test_lt_refusals(native, tmp_path):
    m, w = load(native, tmp_path, "tied1.mmf")
    src = su.golden_bytes("treesA").decode()
    qs, trees = src.split("\n\n", 1)
    first_q = qs.splitlines()[0]
    assert "'L_Vowel'" in trees and '"ST_b_2_1"' in trees and "\nb[2]\n" in trees
    node_line = re.search(r"(?m)^  -1 .*$", trees).group(0)
    cases = {
        "twice": (first_q + "\n" + src, "question name L_Vowel invalid", EINVAL),
        "quest": (qs + "\n\n" + trees.replace("'L_Vowel'", "'Nope'", 1), "Question Nope not recognised", EMODEL),
        "macro": (qs + "\n\n" + trees.replace('"ST_b_2_1"', '"ST_zz"', 1), "Macro ST_zz not recognised", EMODEL),
        "node": (qs + "\n\n" + trees.replace(node_line, node_line.replace("  -1 ", " -77 ", 1), 1), "Node -77 not in tree", EINVAL),
        "noquest": (trees, "Questions Expected", EINVAL),
        "model": (qs + "\n\n" + trees.replace("\nb[2]\n", "\nb\n", 1), r"b is a model tree .*model trees are not built", EMODEL),
        "notrees": (qs + "\n", "holds no trees", EINVAL),
        "open": (src[:src.rindex("}")], "is not closed by }", EIO),
    }
    for name, (text, reason, code) in cases.items():
        p = os.path.join(w, "bad_" + name)
        with open(p, "w") as f:
            f.write(text)
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            m.load_trees(p)
        assert e.value.rc == code, name
        assert m.trees() == []                                                    # a refused file leaves nothing behind
    with pytest.raises(native.HtkAmdError, match="cannot open"):
        m.load_trees(os.path.join(w, "nothing"))
    with pytest.raises(native.HtkAmdError, match="no trees are held"):
        m.save_trees(os.path.join(w, "out"))
    m.load_trees(os.path.join(w, "treesA"))
    with pytest.raises(native.HtkAmdError, match="question name L_Vowel invalid") as e:     # the questions are held already: HHEd's 2661
        m.load_trees(os.path.join(w, "treesA"))
    assert e.value.rc == EINVAL and len(m.trees()) == 27


def co_set(native, tmp_path, extra=""):
    """a, b: everything shared; c: another state; d, e: the state of a with matrices of their own that hold T1's very values."""
    text = HDR + extra + '~t "T1"\n' + MAT + '~s "S1"\n' + state("0 0") + '~s "S2"\n' + state("1 0")
    for name, st, tr in (("a", "S1", '~t "T1"\n'), ("b", "S1", '~t "T1"\n'), ("c", "S2", '~t "T1"\n'), ("d", "S1", MAT), ("e", "S1", MAT)):
        text += hmm(name, '~s "%s"\n' % st, tr)
    (tmp_path / "co.mmf").write_text(text)
    return native.Mmf(files=[str(tmp_path / "co.mmf")])


def test_co_on_hand_made_sets(native, tmp_path):
    m = co_set(native, tmp_path)
    names = list(m.phys_names)
    scan = [names[i] for i in native.hmm_scan_order(names)]
    first, second = [n for n in scan if n in ("a", "b")]
    assert m.compact(str(tmp_path / "list")) == (5, 4)
    assert sorted(m.phys_names) == sorted(set(names) - {second})                 # the first of the group in the table's scan stays
    assert m.logical[second] == m.logical[first] == m.phys_names.index(first)
    assert m.logical["d"] != m.logical["e"]                                       # equal values, but not the same matrix
    # SaveHMMList: the logical names in the table's order, the physical name behind a name that is not its own
    assert (tmp_path / "list").read_text().splitlines() == [n + (" " + first if n == second else "") for n in scan]
    m.write(m.packed(), one_file=str(tmp_path / "out.mmf"))
    out = (tmp_path / "out.mmf").read_text()
    assert re.findall(r'~h "(\w)"', out) == [n for n in scan if n != second]
    m2 = native.Mmf([str(tmp_path / "out.mmf")], hmm_list=str(tmp_path / "list"))   # the compacted set and its list load again
    assert m2.desc.numPhys == 4 and len(m2.logical) == 5 and m2.phys_names[m2.logical[second]] == first
    assert m2.compact() == (5, 4)                                                 # nothing left to merge


def test_co_equivalent_states_need_shared_vectors(native, tmp_path):
    """Two states that are not one macro count as one only in a set with ~u and ~v macros (or ~m), and then when they name the same
    vectors (EquivState); states with equal values in vectors of their own never do."""
    def build(shared):
        text = HDR + '~u "m1"\n<MEAN> 2\n0 0\n~v "v1"\n<VARIANCE> 2\n1 1\n~t "T1"\n' + MAT
        body = '~u "m1"\n~v "v1"\n' if shared else state("0 0")
        text += '~s "S1"\n' + body + '~s "S2"\n' + body + hmm("a", '~s "S1"\n', '~t "T1"\n') + hmm("b", '~s "S2"\n', '~t "T1"\n')
        p = tmp_path / ("eq%d.mmf" % shared)
        p.write_text(text)
        return native.Mmf(files=[str(p)])
    assert build(1).compact() == (2, 1)
    assert build(0).compact() == (2, 2)


def test_compact_of_the_uncompacted_set_is_hhed_s(native, tmp_path):
    """Case A's set after AU, loaded from its file: CO gives HHEd's list and set byte for byte (HHEd run on the same file), and the counts."""
    m, w = load(native, tmp_path, "synthA_au.mmf", lst="full")
    assert m.compact(os.path.join(w, "tiedlist")) == (su.COUNTS["caseA_co"]["CO"]["logical"], su.COUNTS["caseA_co"]["CO"]["physical"])
    m.write(m.packed(), one_file=os.path.join(w, "out.mmf"))
    su.same(open(os.path.join(w, "tiedlist"), "rb").read(), su.golden_bytes("tiedlistA_co"), "tied list")
    su.same(open(os.path.join(w, "out.mmf"), "rb").read(), su.golden_bytes("synthA_co.mmf"), "compacted set")
    assert su.golden_bytes("tiedlistA_co") == su.golden_bytes("tiedlistA")          # ... which is the list of the one-run recipe


def test_parse_script_keeps_lt_au_co_behind_the_keyword(native):
    from htk_amd import treeclust
    text = "LT trees\nQS 'q' { \"a-*\" }\nAU \"full list\"\nCO tiedlist\nST out\n"
    sc = treeclust.parse_script(text, synth=True)
    assert [c[0] for c in sc.commands] == ["LT", "QS", "AU", "CO", "ST"]
    assert sc.commands[0] == ("LT", "trees") and sc.commands[2] == ("AU", "full list") and sc.commands[3] == ("CO", "tiedlist")
    for cmd in ("LT trees", "AU full", "CO tiedlist"):
        with pytest.raises(native.HtkAmdError) as e:
            treeclust.parse_script(cmd + "\n")
        assert str(e.value) == "edit script: command %s is not supported (only RO, TR, QS, TB, ST, TC, NC, TI, LS: state clustering and tying)" % cmd[:2]
    for kw in (False, True):
        with pytest.raises(native.HtkAmdError, match="command MU is not supported"):
            treeclust.parse_script("MU 2 {*.state[2-4].mix}\n", synth=kw)
    with pytest.raises(native.HtkAmdError, match="AU: file name expected"):
        treeclust.parse_script("AU\n", synth=True)


def test_add_unseen_refusals_and_no_device(native, tmp_path):
    m, w = load(native, tmp_path, "tied1.mmf")
    with pytest.raises(native.HtkAmdError, match="there are no existing trees"):
        m.add_unseen(os.path.join(w, "full"))
    m.load_trees(os.path.join(w, "treesA"))
    for name, text, reason in (("phys", "a-b+c x-y+z\n", r"has the physical name x-y\+z"), ("twice", "a-b+c\nb-b+c\na-b+c\n", r"lists model a-b\+c twice"),
                               ("empty", "\n", "lists no model"), ("long", "a-" + "b" * 100 + "+c\n", r"has 104 characters \(at most 99")):
        with open(os.path.join(w, name), "w") as f:
            f.write(text)
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            m.add_unseen(os.path.join(w, name))
        assert e.value.rc == EINVAL
    # the reference's failures, found before a device is needed: no proto (case E), no tree for a state (treesE2 lacks b[4])
    with pytest.raises(native.HtkAmdError, match="no proto for sil in hSet") as e:
        m.add_unseen(os.path.join(w, "fullE"))
    assert su.COUNTS["caseE_error"].endswith(str(e.value).split("mmf_add_unseen: ")[-1])
    m2, w2 = load(native, tmp_path, "tied1.mmf")
    m2.load_trees(os.path.join(w2, "treesE2"))
    with pytest.raises(native.HtkAmdError, match="cannot find tree for a-b\\+a state 4") as e:
        m2.add_unseen(os.path.join(w2, "full"))
    assert su.COUNTS["caseE2_error"].endswith(str(e.value).split("mmf_add_unseen: ")[-1])
    assert len(m.phys_names) == 161                                               # a refused call changes nothing
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        m.add_unseen(os.path.join(w, "full"))
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        native.name_question_answers(["a-b+c"], [("q", ["a-*"])])


def test_trees_reader_under_asan_ubsan(tmp_path):
    """The reader takes arbitrary text: a stand-alone program over the host files, built with the sanitizers, over the committed trees
    files and over truncated and mangled ones -- every file is taken or refused, nothing else."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan in this toolchain")
    root = tu.ROOT
    exe = str(tmp_path / "parse_main")
    srcs = [os.path.join(root, "tests", "treesynth_parse_main.c")] + sorted(glob.glob(os.path.join(root, "htk_amd", "host", "*.c")))
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(root, "include"), "-o", exe] + srcs + ["-lm"])
    w = su.workdir(tmp_path, "tied1.mmf")
    src = su.golden_bytes("treesA")
    files = {"treesA": src, "lt_st": su.golden_bytes("treesA.lt_st"), "trees3": tu.golden_bytes("trees3"), "hand": tu.golden_bytes("trees_hand.expected"), "empty": b"",
             "qs_only": src.split(b"\n\n")[0], "binary": bytes(range(256)) * 8, "quote": src.replace(b'"ST_a_2_1"', b'"ST_a_2_1', 1),
             "brace": src.replace(b"{", b"", 1), "nobrace": src.replace(b" }", b"", 1), "escape": src.replace(b"'L_Vowel'", b"'L_\\126owel\\", 1),
             "bignode": src.replace(b"  -1 ", b" -99999999 ", 1), "posnode": src.replace(b"  -1 ", b"  1 ", 1), "longtok": b"QS 'q' { \"" + b"x" * 9000 + b"\" }\n\na[2]\n \"ST_a_2_1\"\n",
             "selfloop": b"QS 'q' { \"a-*\" }\n\na[2]\n{\n 0 'q' 0 \"ST_a_2_1\"\n}\n", "twoparents": b"QS 'q' { \"a-*\" }\n\na[2]\n{\n 0 'q' -1 -1\n -1 'q' \"ST_a_2_1\" \"ST_a_2_1\"\n}\n"}
    for cut in (1, 17, 300, 1500, 1601, 4000, len(src) - 2):
        files["cut%d" % cut] = src[:cut]
    paths = []
    for n, data in files.items():
        paths.append(os.path.join(w, "f_" + n))
        with open(paths[-1], "wb") as f:
            f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, os.path.join(w, "in.mmf"), os.path.join(w, "seen")] + paths, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if re.match(r"-?\d+ /", ln)]     # (a reason may quote a token with a line break in it)
    assert len(lines) == len(paths)
    taken = [os.path.basename(ln.split()[1].rstrip(":")) for ln in lines if ln.startswith("0 ")]
    # (the leaves of trees3 are macros of this set, too; the hand-made file names others; the last cut only loses the empty lines at the end)
    assert taken == ["f_treesA", "f_lt_st", "f_trees3", "f_cut%d" % (len(src) - 2)], lines
    assert open(os.path.join(w, "f_treesA.saved"), "rb").read() == su.golden_bytes("treesA.lt_st")
