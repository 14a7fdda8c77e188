"""Helpers shared by the scoring tests: the fixture runs, a plain restatement of the reference's alignment grid, and a parser that turns
HResults's text back into the numbers it was printed from."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_results_golden import OUT as GOLD, RUNS, corner_pairs, norm_pairs  # noqa: E402,F401

HIT, SUB, DEL, INS = 0, 1, 2, 3
DIAG, VERT, HOR = 0, 1, 2


def strip_date(text):
    lines = text.splitlines(keepends=True)
    assert sum(l.startswith("  Date: ") for l in lines) <= 1
    return "".join(l for l in lines if not l.startswith("  Date: "))


def grid_align(ref, test, nist):
    """The reference's grid on id lists (0 = the null class), row by row as it fills it: the last cell's counters and the triples
    (op, refId, testId) its traceback yields, steps with a null label dropped."""
    sub, dele, ins = (4, 3, 3) if nist else (10, 7, 7)
    R, T = len(ref), len(test)
    zero = dict(score=0, ins=0, sub=0, hit=0)
    zero["del"] = 0
    g = [[None] * (R + 1) for _ in range(T + 1)]
    g[0][0] = dict(zero, dir=None)
    for i in range(1, T + 1):
        c = dict(g[i - 1][0], dir=HOR)
        if test[i - 1] != 0:
            c["score"] += ins; c["ins"] += 1
        g[i][0] = c
    for j in range(1, R + 1):
        c = dict(g[0][j - 1], dir=VERT)
        if ref[j - 1] != 0:
            c["score"] += dele; c["del"] += 1
        g[0][j] = c
    for i in range(1, T + 1):
        tn = test[i - 1] == 0
        for j in range(1, R + 1):
            rn = ref[j - 1] == 0
            up, dg, lf = g[i - 1][j], g[i - 1][j - 1], g[i][j - 1]
            if rn and not tn:
                c = dict(lf, dir=VERT)
            elif tn and not rn:
                c = dict(up, dir=HOR)
            else:
                h, d, v = up["score"], dg["score"], lf["score"]
                same = ref[j - 1] == test[i - 1]
                if not rn:
                    h += ins; v += dele; d += 0 if same else sub
                if nist:
                    go = VERT if (v <= d and v <= h) else (DIAG if d <= h else HOR)
                else:
                    go = DIAG if (d <= h and d <= v) else (HOR if h < v else VERT)
                c = dict({DIAG: dg, HOR: up, VERT: lf}[go], dir=go)
                c["score"] = {DIAG: d, HOR: h, VERT: v}[go]
                if not rn:
                    c[{DIAG: "hit" if same else "sub", HOR: "ins", VERT: "del"}[go]] += 1
            g[i][j] = c
    out, i, j = [], T, R
    while i > 0 or j > 0:
        go = g[i][j]["dir"]
        if go == DIAG:
            r, t = ref[j - 1], test[i - 1]; i -= 1; j -= 1
            if r != 0 and t != 0:
                out.append((HIT if r == t else SUB, r, t))
        elif go == VERT:
            r = ref[j - 1]; j -= 1
            if r != 0:
                out.append((DEL, r, -1))
        else:
            t = test[i - 1]; i -= 1
            if t != 0:
                out.append((INS, -1, t))
    return g[T][R], out[::-1]


def parse_output(text, label_id):
    """HResults's standard output -> dict(files=[(name, [H, D, S, I, N])] from the -f lines, aligned={lab file: (rec file, triples)} from
    the -t blocks, totals=[H, D, S, I, N, sentences, correct], conf={(row, column): count} with "Ins" / "Del" as names).
    label_id: name -> id, for the triples."""
    lines = text.splitlines()
    out = dict(files=[], aligned={}, totals=None, conf=None, rec=[], ref=None)
    k = 0
    while k < len(lines):
        l = lines[k]
        m = re.match(r"(\S+):\s+\S+\(\s*\S+\)\s+\[H=\s*(\d+), D=\s*(\d+), S=\s*(\d+), I=\s*(\d+), N=\s*(\d+)\]$", l)
        if m:
            out["files"].append((m.group(1), [int(x) for x in m.groups()[1:]]))
        elif l.startswith("Aligned transcription: "):
            lab, rec = l[len("Aligned transcription: "):].split(" vs ")
            a, b = lines[k + 1], lines[k + 2]
            assert a.startswith(" LAB: ") and b.startswith(" REC: ") and len(a) == len(b)
            pos, tr = 6, []
            while pos < len(a):
                x, y = a[pos:].split(" ")[0], b[pos:].split(" ")[0]
                tr.append((DEL, label_id(x), -1) if not y else (INS, -1, label_id(y)) if not x else (HIT if label_id(x) == label_id(y) else SUB, label_id(x), label_id(y)))
                pos += max(len(x), len(y)) + 1
            out["aligned"][lab] = (rec, tr)
            k += 2
        elif l.startswith("  Ref : "):
            out["ref"] = l[8:]
        elif l.startswith("  Rec : ") or l.startswith("      : "):
            out["rec"].append(l[8:])
        elif l.startswith("SENT: "):
            m = re.search(r"\[H=(\d+), S=(\d+), N=(\d+)\]", l)
            sent = (int(m.group(3)), int(m.group(1)))
        elif l.startswith("WORD: "):
            m = re.search(r"\[H=(\d+), D=(\d+), S=(\d+), I=(\d+), N=(\d+)\]", l)
            out["totals"] = [int(x) for x in m.groups()] + list(sent)
        elif "Confusion Matrix" in l:
            head = []
            k += 1
            while not lines[k].rstrip().endswith("%e]"):
                head.append(lines[k]); k += 1
            head.append(lines[k][:lines[k].index(" Del [")])
            ncol = (max(len(h) for h in head) - 5 + 3) // 4
            cols = ["".join(h[5 + 4 * c + 2:5 + 4 * c + 3] for h in head).strip() for c in range(ncol)]
            conf = {}
            k += 1
            while not lines[k].startswith("Ins "):
                row = lines[k][:4].strip()
                cells = [int(lines[k][5 + 4 * c:9 + 4 * c]) for c in range(ncol + 1)]
                for c, name in enumerate(cols):
                    conf[(row, name)] = cells[c]
                conf[(row, "Del")] = cells[ncol]
                k += 1
            for c, name in enumerate(cols):
                conf[("Ins", name)] = int(lines[k][4 + 4 * c:8 + 4 * c])
            out["conf"] = conf
        k += 1
    return out
