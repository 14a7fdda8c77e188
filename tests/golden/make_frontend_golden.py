#!/usr/bin/env python3
"""Golden vectors for the PLP / FBANK / MELSPEC kinds of the waveform front end: the reference's HCopy (oracle/_ref, built from the
reference tree by oracle/Makefile) codes the committed tests/golden/wave/test.wav with one configuration per case; the configuration
texts (frontend_<case>.conf) and the outputs (test_<KIND>.<case>.htk) are committed next to it.  A second set codes a batch of 8
synthetic waveforms of different lengths (batch_waves / batch_<case> in frontend_batch.npz) for the per-utterance frame offsets.

    make -C oracle _ref/HCopy && python tests/golden/make_frontend_golden.py
"""
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "wave")
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")

COMMON = "SOURCEFORMAT = WAV\nSOURCERATE = 625\nWINDOWSIZE = 250000.0\nTARGETRATE = 100000.0\nPREEMCOEF = 0.97\nUSEHAMMING = T\n"
# case -> (TARGETKIND, the settings that matter)
CASES = {
    "a": ("PLP_0_D_A", "NUMCHANS = 26\nNUMCEPS = 12\nLPCORDER = 12\nUSEPOWER = T\nCEPLIFTER = 22\nENORMALISE = F\n"),
    "b": ("PLP_E_D_A_Z", "NUMCHANS = 26\nNUMCEPS = 14\nLPCORDER = 16\nUSEPOWER = T\nCEPLIFTER = 22\nENORMALISE = T\n"),
    "c": ("PLP_0", "NUMCHANS = 24\nNUMCEPS = 12\nLPCORDER = 12\nUSEPOWER = F\nCEPLIFTER = 22\n"),
    "d": ("FBANK_E_D_A", "NUMCHANS = 40\nENORMALISE = F\n"),
    "e": ("FBANK", "NUMCHANS = 24\nZMEANSOURCE = T\n"),
    "f": ("MELSPEC", "NUMCHANS = 26\n"),
}
BATCH_CASES = ("a", "d")


def conf_text(case):
    kind, extra = CASES[case]
    return COMMON + "TARGETKIND = %s\n" % kind + extra


def out_name(case):
    return "test_%s.%s.htk" % (CASES[case][0], case)


def batch_waves(seed=13):
    """8 waveforms of different lengths (two of a single frame: HCopy writes no empty file), 16 kHz int16."""
    rng = np.random.default_rng(seed)
    lens = [16000, 3999, 400, 401, 8123, 12345, 560, 20011]
    out = []
    for i, n in enumerate(lens):
        t = np.arange(n) / 16000.0
        x = 2500 * np.sin(2 * np.pi * (300 + 170 * i) * t) + 1200 * np.sin(2 * np.pi * 2100 * t) + rng.normal(0, 600 + 100 * i, n)
        out.append(x.clip(-32768, 32767).astype("<i2"))
    return out


def write_wav(path, x):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.asarray(x, "<i2").tobytes())


def hcopy(exe, conf, src, dst):
    subprocess.check_call([exe, "-C", conf, src, dst], stdout=subprocess.DEVNULL)


def read_htk(path):
    """HTK parameter file (big-endian header + float32 rows, HCopy's trailing CRC ignored) -> (rows, kind code without _K)."""
    raw = open(path, "rb").read()
    n, _per, size, kind = (int(v) for v in np.frombuffer(raw[:12], ">i4,>i4,>i2,>i2")[0])
    return np.frombuffer(raw[12:12 + n * size], ">f4").reshape(n, size // 4).astype(np.float32), kind & ~0o10000


def code_batch(exe, case, waves, d):
    """HCopy on every wave of `waves` with case `case`'s configuration: the rows of all of them, back to back, and the frame offsets."""
    conf = os.path.join(d, "batch_%s.conf" % case)
    open(conf, "w").write(conf_text(case))
    rows, off = [], [0]
    for i, x in enumerate(waves):
        src, dst = os.path.join(d, "b%d.wav" % i), os.path.join(d, "b%d_%s.htk" % (i, case))
        write_wav(src, x)
        hcopy(exe, conf, src, dst)
        r, _ = read_htk(dst)
        rows.append(r); off.append(off[-1] + r.shape[0])
    return np.concatenate(rows), np.asarray(off, np.int32)


if __name__ == "__main__":
    if not os.path.exists(HCOPY):
        sys.exit("needs %s (make -C oracle _ref/HCopy)" % HCOPY)
    wav = os.path.join(OUT, "test.wav")
    for case in CASES:
        conf = os.path.join(OUT, "frontend_%s.conf" % case)
        open(conf, "w").write(conf_text(case))
        hcopy(HCOPY, conf, wav, os.path.join(OUT, out_name(case)))
        r, k = read_htk(os.path.join(OUT, out_name(case)))
        print(case, CASES[case][0], r.shape, "kind", k)
    waves = batch_waves()
    arrs = {}
    with tempfile.TemporaryDirectory() as d:
        for case in BATCH_CASES:
            rows, off = code_batch(HCOPY, case, waves, d)
            arrs["batch_%s" % case] = rows; arrs["batch_%s_off" % case] = off
    np.savez_compressed(os.path.join(OUT, "frontend_batch.npz"), **arrs)
    print({k: v.shape for k, v in arrs.items()})
