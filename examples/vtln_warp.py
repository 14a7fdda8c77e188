#!/usr/bin/env python3
"""VTLN warp factors by grid search, on the device.

    python examples/vtln_warp.py -C config -H MMF --scp files.scp [--factors 0.88:1.12:13] [--lcut 300 --ucut 3400] [-o warps.txt] hmmlist

files.scp names one WAV file and its speaker per line (`path speaker`); the transcription of a file is the label file beside it
(`path` with the extension .lab, a model name per line).  config is an HTK configuration for the waveform front end (TARGETKIND,
WINDOWSIZE, NUMCHANS, ...; SOURCERATE is taken from the WAV headers when it is absent).

Every file is coded under every factor in ONE call (FrontEnd.compute_grid: window, FFT and magnitudes once per frame, the mel bins
once per factor), every table is force-aligned against the transcriptions (Viterbi), the utterances' log likelihoods are summed per
speaker and factor, and every speaker gets the factor with the highest sum.  The `speaker alpha` lines go to -o (or stdout); the
batch is then recoded with every file under its speaker's factor (FrontEnd.compute with warp_index).

As in the usual recipe the likelihoods are compared as they are: there is NO Jacobian term for the warp, so the choice leans
towards factors that compress the spectrum where the models are broad.  Compensating for that is outside this example.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402

# configuration variable -> frontend_config keyword
_VARS = {"SOURCERATE": ("sampPeriod", float), "WINDOWSIZE": ("winDur", float), "TARGETRATE": ("frPeriod", float),
         "NUMCHANS": ("numChans", int), "NUMCEPS": ("numCeps", int), "CEPLIFTER": ("cepLifter", int), "PREEMCOEF": ("preEmph", float),
         "USEHAMMING": ("useHam", bool), "USEPOWER": ("usePower", bool), "ZMEANSOURCE": ("zMeanSource", bool),
         "ENORMALISE": ("eNormalise", bool), "RAWENERGY": ("rawEnergy", bool), "LPCORDER": ("lpcOrder", int),
         "COMPRESSFACT": ("compressFact", float), "CEPSCALE": ("cepScale", float), "LOFREQ": ("loFreq", float), "HIFREQ": ("hiFreq", float),
         "DELTAWINDOW": ("delWin", int), "ACCWINDOW": ("accWin", int), "SILFLOOR": ("silFloor", float), "ESCALE": ("eScale", float)}


def read_config(path):
    """(TARGETKIND, keyword arguments of capi.frontend_config) of an HTK configuration file; HParm's defaults for what it does not set."""
    kw, kind = {"usePower": False, "numChans": 20, "winDur": 256000.0}, "MFCC_0_D_A"
    for line in open(path):
        line = line.split("#")[0]
        if "=" not in line:
            continue
        k, v = (x.strip() for x in line.split("="))
        k = k.split(":")[-1].strip().upper()
        if k == "TARGETKIND":
            kind = v
        elif k in _VARS:
            name, typ = _VARS[k]
            kw[name] = (v[0] in "Tt") if typ is bool else typ(v)
    return kind, kw


def score_tables(model, dX, frameOff, labOff, labs, tables, cols):
    """[tables x utterances] log likelihoods of the forced alignments of `tables` feature tables lying behind one another in dX"""
    vit = capi.Viterbi(model)
    F = int(frameOff[-1])
    out = np.empty((tables, len(frameOff) - 1))
    for w in range(tables):
        res = vit.align(dX.ptr.value + 4 * w * F * cols, frameOff, labOff, labs)
        out[w] = [r["total"] if r["status"] == 1 else -np.inf for r in res]
    vit.close()
    return out


def pick_warps(cfg, waves, speakers, model, labOff, labs, warps, grid=True):
    """The warp of `warps` with the highest summed alignment likelihood for every speaker: ({speaker: index}, scores [warps x utterances]).
    grid: all warps in one compute_grid call; otherwise one single-warp front end and call per warp (the same numbers, the slow way)."""
    if grid:
        fe = capi.FrontEnd(cfg, warps=warps)
        dX, frameOff = fe.compute_grid(waves)
        scores = score_tables(model, dX, frameOff, labOff, labs, len(warps), fe.cols)
        fe.close()
    else:
        scores = np.empty((len(warps), len(waves)))
        for w, warp in enumerate(warps):
            fe = capi.FrontEnd(cfg, warps=[warp])
            dX, frameOff = fe.compute(waves)
            scores[w] = score_tables(model, dX, frameOff, labOff, labs, 1, fe.cols)[0]
            fe.close()
    best = {}
    for spk in sorted(set(speakers)):
        mine = [u for u, s in enumerate(speakers) if s == spk]
        best[spk] = int(np.argmax(scores[:, mine].sum(axis=1)))
    return best, scores


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-C", dest="config", required=True, help="HTK configuration of the waveform front end")
    ap.add_argument("-H", dest="mmf", required=True, action="append", help="model set (repeatable)")
    ap.add_argument("--scp", required=True, help="lines `file.wav speaker`; transcriptions in file.lab beside each")
    ap.add_argument("--factors", default="0.88:1.12:13", help="lowest:highest:count of the warp factors tried (default 0.88:1.12:13)")
    ap.add_argument("--lcut", type=float, default=300.0, help="WARPLCUTOFF (Hz)")
    ap.add_argument("--ucut", type=float, default=3400.0, help="WARPUCUTOFF (Hz)")
    ap.add_argument("-o", dest="out", help="where the `speaker alpha` lines go (default: stdout); no Jacobian term is applied")
    ap.add_argument("--features", help="write the recoded batch here (.npz: feats, frameOff)")
    ap.add_argument("hmmlist")
    a = ap.parse_args(argv)

    lo, hi, n = a.factors.split(":")
    warps = [(float(f), a.lcut, a.ucut) for f in np.linspace(float(lo), float(hi), int(n))]
    files, speakers = zip(*[line.split()[:2] for line in open(a.scp) if line.strip()])
    kind, kw = read_config(a.config)
    waves, period = [], None
    for f in files:
        x, per = capi.wave_read(f)
        waves.append(x); period = period or per
    kw.setdefault("sampPeriod", period)
    cfg = capi.frontend_config(kind, **kw)

    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    mmf = capi.Mmf(a.mmf, hmm_list=a.hmmlist)
    mmf.refuse_input_xform("vtln_warp")
    model = capi.Model(mmf.packed())
    seqs = [[mmf.logical[l.split()[-1]] for l in open(os.path.splitext(f)[0] + ".lab") if l.strip()] for f in files]
    labOff = capi.offsets([len(q) for q in seqs])
    labs = np.concatenate(seqs).astype(np.int32)

    best, _ = pick_warps(cfg, waves, speakers, model, labOff, labs, warps)
    out = open(a.out, "w") if a.out else sys.stdout
    for spk in sorted(best):
        out.write("%s %.4f\n" % (spk, warps[best[spk]][0]))
    if a.out:
        out.close()
    fe = capi.FrontEnd(cfg, warps=warps)
    feats, frameOff = fe.compute_host(waves, warp_index=[best[s] for s in speakers])
    fe.close()
    if a.features:
        np.savez(a.features, feats=feats, frameOff=frameOff)
    return best


if __name__ == "__main__":
    main()
