"""Wall time of HHEd's AU + CO (unseen triphones from the trees, then the compacted set) on a synthetic tied set over P phones and the full
list of P^3 triphones: the library (AU's two kernels on the device, the wiring and CO on the host) and, where oracle/_ref/HHEd exists,
the reference's HHEd on one core over the same files ("LT trees AU full CO tiedlist", and an empty script for its load + save share).
Prints one JSON line.

    python tools/synth_bench.py [--phones 40] [--contexts 200] [--dim 13] [--questions 200] [--reps 5]

The set is tools/tree_bench.py's (tied here by RO / QS / TB on the device first).  AU and CO are timed on a freshly loaded copy of the tied
set per repetition (both change the set); the first repetition warms the device up and is not counted; the medians are reported.  The
kernels' own times are the device's events around each launch (htkamd_synth_last_kernel_ms)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from htk_amd import capi, treeclust      # noqa: E402
import tree_bench                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, default=40); ap.add_argument("--contexts", type=int, default=200)
    ap.add_argument("--dim", type=int, default=13); ap.add_argument("--questions", type=int, default=200); ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        J = lambda n: os.path.join(d, n)      # noqa: E731
        H = tree_bench.write_inputs(d, a.phones, a.contexts, a.dim, a.questions)
        phones = ["p%02d" % k for k in range(a.phones)]
        with open(J("full"), "w") as f:
            f.write("".join("%s-%s+%s\n" % (l, c, r) for c in phones for l in phones for r in phones))
        m = capi.Mmf([J("hmmdefs")], hmm_list=J("hmmlist"))
        treeclust.run_script(m, treeclust.parse_script(open(J("tree.hed")).read()), base_dir=d)
        m.write(m.packed(), one_file=J("tied.mmf"))
        res = dict(seen=H, names=a.phones ** 3, questions=a.questions, trees=3 * a.phones, tied_states=int(m.desc.numStates))
        au, co, k1, k2 = [], [], [], []
        for rep in range(a.reps + 1):
            m = capi.Mmf([J("tied.mmf")], hmm_list=J("hmmlist"))
            m.load_trees(J("trees"))
            t0 = time.perf_counter()
            seen, unseen = m.add_unseen(J("full"))
            t1 = time.perf_counter()
            nlog, nphys = m.compact(J("tiedlist_dev"))
            t2 = time.perf_counter()
            ms = capi.synth_last_kernel_ms()
            if rep:
                au.append(t1 - t0); co.append(t2 - t1); k1.append(ms[0]); k2.append(ms[1])
            if rep == a.reps:
                m.write(m.packed(), one_file=J("synth_dev.mmf"))
            m.close()
        med = statistics.median
        res.update(unseen=unseen, physical=nphys, au_s=round(med(au), 4), co_s=round(med(co), 4), k_name_answers_ms=round(med(k1), 3), k_tree_descend_ms=round(med(k2), 3),
                   kernel_share_of_au=round((med(k1) + med(k2)) / 1000.0 / med(au), 4), reps=a.reps)
        hhed = os.path.join(ROOT, "oracle", "_ref", "HHEd")
        if os.path.exists(hhed):
            for key, text in (("hhed_au_co_s", "LT trees\nAU full\nCO tiedlist_ref\n"), ("hhed_load_save_s", "TR 0\n")):
                with open(J("s.hed"), "w") as f:
                    f.write(text)
                t0 = time.perf_counter()
                subprocess.run([hhed, "-H", "tied.mmf", "-w", "synth_ref.mmf" if "AU" in text else "copy_ref.mmf", "s.hed", "hmmlist"], cwd=d, check=True, stdout=subprocess.DEVNULL)
                res[key] = round(time.perf_counter() - t0, 3)
            res["same_bytes"] = bool(open(J("synth_dev.mmf"), "rb").read() == open(J("synth_ref.mmf"), "rb").read() and
                                     open(J("tiedlist_dev"), "rb").read() == open(J("tiedlist_ref"), "rb").read())
        print(json.dumps(res))


if __name__ == "__main__":
    main()
