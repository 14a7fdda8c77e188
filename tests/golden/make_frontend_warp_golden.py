#!/usr/bin/env python3
"""Golden vectors for the waveform front end under VTLN frequency warping (WARPFREQ, WARPLCUTOFF, WARPUCUTOFF): the reference's HCopy
(oracle/_ref, built from the reference tree by oracle/Makefile) on batches of short synthetic waveforms (case_waves: seeded, not
committed), every case under several warp factors, alpha = 1 among them.

The cases: factors 0.88 .. 1.12 with the cut-offs 300 / 3400 at 16 kHz for every kind and lane layout (MFCC_0_D_A at 26 channels: two
frames per wavefront; MFCC_0 and FBANK at 40: one; MELSPEC; PLP_0_D_A, whose equal-loudness curve sits at the warped centres;
MFCC_E_D_A_Z), equal cut-offs, a band narrowed by LOFREQ / HIFREQ (minFreq != 0), 8 kHz, a 128-point FFT, and a ragged batch of 1, 2,
3, 7 and 40 frames for the calls that give every utterance another warp.

The rows of a batch under factor alpha, back to back, go into tests/golden/wave/frontend_warp.npz as <case>_a<100 alpha>, its frame
offsets as <case>_off; the configuration texts without the three warp variables into tests/golden/wave/frontend_warp.conf (one
"[case]" section each; the variables are warp_text's).  tests/golden/wave/test_MFCC_0_D_A.warp112.mfc is tests/golden/wave/test.wav
coded with alpha = 1.12, for the drivers' test.

    make -C oracle _ref/HCopy && python tests/golden/make_frontend_warp_golden.py
"""
import os
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_frontend_golden import hcopy, read_htk  # noqa: E402
from make_frontend_geom_golden import write_npz, write_wav, read_confs as _read_confs  # noqa: E402
from make_wav_labels_golden import FRONT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "wave")
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")
NPZ = os.path.join(OUT, "frontend_warp.npz")
CONF = os.path.join(OUT, "frontend_warp.conf")
WAV = os.path.join(OUT, "test.wav")
WAV_WARP = (1.12, 300.0, 3400.0)                          # the warp of the committed parameter file of test.wav
WAV_PARM = os.path.join(OUT, "test_MFCC_0_D_A.warp112.mfc")

COMMON = "SOURCEFORMAT = WAV\nPREEMCOEF = 0.97\nUSEHAMMING = T\nTARGETRATE = 100000.0\n"
MFCC = "NUMCHANS = 26\nNUMCEPS = 12\nCEPLIFTER = 22\nENORMALISE = F\n"
FIVE = (0.88, 0.94, 1.0, 1.06, 1.12)
THREE = (0.88, 1.0, 1.12)
FRAMES = (1, 2, 7, 3)
RAGGED = (1, 2, 3, 7, 40)

# case -> (rate in Hz, WINDOWSIZE, TARGETKIND, the settings that matter, (WARPLCUTOFF, WARPUCUTOFF), factors, frames per utterance)
CASES = {
    "mfcc26": (16000, 250000.0, "MFCC_0_D_A", MFCC, (300.0, 3400.0), FIVE, FRAMES),
    "mfcc40": (16000, 250000.0, "MFCC_0", "NUMCHANS = 40\nNUMCEPS = 12\nCEPLIFTER = 22\n", (300.0, 3400.0), FIVE, FRAMES),
    "fbank40": (16000, 250000.0, "FBANK", "NUMCHANS = 40\n", (300.0, 3400.0), FIVE, FRAMES),
    "melspec": (16000, 250000.0, "MELSPEC", "NUMCHANS = 26\n", (300.0, 3400.0), FIVE, FRAMES),
    "plp": (16000, 250000.0, "PLP_0_D_A", "NUMCHANS = 26\nNUMCEPS = 12\nLPCORDER = 12\nUSEPOWER = T\nCEPLIFTER = 22\nENORMALISE = F\n",
            (300.0, 3400.0), FIVE, FRAMES),
    "mfcc_ez": (16000, 250000.0, "MFCC_E_D_A_Z", "NUMCHANS = 26\nNUMCEPS = 12\nCEPLIFTER = 22\nENORMALISE = T\n", (300.0, 3400.0), FIVE, FRAMES),
    "eqcut": (16000, 250000.0, "MFCC_0_D_A", MFCC, (1500.0, 1500.0), THREE, FRAMES),                 # WARPLCUTOFF == WARPUCUTOFF
    "band": (16000, 250000.0, "MFCC_0_D_A", MFCC + "LOFREQ = 60\nHIFREQ = 7800\n", (300.0, 3400.0), THREE, FRAMES),     # minFreq != 0
    "r8k": (8000, 250000.0, "MFCC_0_D_A", MFCC, (200.0, 3000.0), THREE, FRAMES),                   # frSize 200, fftN 256
    "fft128": (8000, 100000.0, "MFCC_0_D_A", MFCC, (200.0, 3000.0), THREE, FRAMES),                # frSize 80, fftN 128
    "ragged": (16000, 250000.0, "MFCC_0_D_A", MFCC, (300.0, 3400.0), FIVE, RAGGED),                # utterance i under factor i: two warps in one pair of frames
}


def key(case, alpha):
    return "%s_a%03d" % (case, int(round(100 * alpha)))


def conf_text(case):
    """the case's configuration without the warp"""
    _, win, kind, extra, _, _, _ = CASES[case]
    return COMMON + "WINDOWSIZE = %.1f\nTARGETKIND = %s\n" % (win, kind) + extra


def warp_text(case, alpha):
    lo, hi = CASES[case][4]
    return "WARPFREQ = %.2f\nWARPLCUTOFF = %.1f\nWARPUCUTOFF = %.1f\n" % (alpha, lo, hi)


def warps(case):
    """the case's (WARPFREQ, WARPLCUTOFF, WARPUCUTOFF) triples, in the order of its factors"""
    lo, hi = CASES[case][4]
    return [(a, lo, hi) for a in CASES[case][5]]


def read_confs():
    return _read_confs(CONF)


def case_waves(case):
    """The case's batch: three sines plus noise at the case's rate, int16, each utterance a few samples longer than its frames need."""
    hz, win, _, _, _, _, frames = CASES[case]
    frSize, frRate = int(win / (1.0e7 / hz)), int(100000.0 / (1.0e7 / hz))
    rng = np.random.default_rng(zlib.crc32(("warp_" + case).encode()))
    out = []
    for i, nf in enumerate(frames):
        n = frSize + (nf - 1) * frRate + int(rng.integers(0, frRate))
        t = np.arange(n) / float(hz)
        x = (2500 * np.sin(2 * np.pi * (250 + 130 * i) * t) + 1500 * np.sin(2 * np.pi * (1300 + 90 * i) * t)
             + 1000 * np.sin(2 * np.pi * 0.4 * hz * t) + rng.normal(0, 500 + 100 * i, n))
        out.append(x.clip(-32768, 32767).astype("<i2"))
    return out


def code_batch(exe, case, alpha, waves, d):
    """HCopy on every wave of `waves` with case `case`'s configuration under factor alpha: the rows, back to back, and the frame offsets."""
    conf = os.path.join(d, "%s.conf" % key(case, alpha))
    open(conf, "w").write(conf_text(case) + warp_text(case, alpha))
    rows, off = [], [0]
    for i, x in enumerate(waves):
        src, dst = os.path.join(d, "%s_%d.wav" % (case, i)), os.path.join(d, "%s_%d.htk" % (key(case, alpha), i))
        write_wav(src, x, CASES[case][0])
        hcopy(exe, conf, src, dst)
        r, _ = read_htk(dst)
        rows.append(r); off.append(off[-1] + r.shape[0])
    return np.concatenate(rows), np.asarray(off, np.int32)


def wav_conf(alpha):
    """the drivers' configuration for tests/golden/wave/test.wav (make_wav_labels_golden.FRONT) under WAV_WARP's cut-offs"""
    return "SOURCEFORMAT = WAV\n" + FRONT + "TARGETKIND = MFCC_0_D_A\nWARPFREQ = %.2f\nWARPLCUTOFF = %.1f\nWARPUCUTOFF = %.1f\n" % (alpha, WAV_WARP[1], WAV_WARP[2])


if __name__ == "__main__":
    if not os.path.exists(HCOPY):
        sys.exit("needs %s (make -C oracle _ref/HCopy)" % HCOPY)
    arrs = {}
    with tempfile.TemporaryDirectory() as d:
        for case in sorted(CASES):
            waves = case_waves(case)
            for alpha in CASES[case][5]:
                rows, off = code_batch(HCOPY, case, alpha, waves, d)
                assert list(np.diff(off)) == list(CASES[case][6]), (case, off)
                arrs[key(case, alpha)] = rows; arrs[case + "_off"] = off
            plain = arrs[key(case, 1.0)]
            for alpha in CASES[case][5]:                # a fixture in which the warp has no effect proves nothing
                if alpha != 1.0:
                    diff = np.abs(arrs[key(case, alpha)] - plain).max()
                    assert diff > 1e-3, (case, alpha, diff)
                    print(case, CASES[case][2], alpha, arrs[key(case, alpha)].shape, "max |warped - plain| %.3g" % diff)
        conf = os.path.join(d, "wav.conf")
        open(conf, "w").write(wav_conf(WAV_WARP[0]))
        hcopy(HCOPY, conf, WAV, WAV_PARM)
        open(conf, "w").write(wav_conf(1.0))
        hcopy(HCOPY, conf, WAV, os.path.join(d, "plain.mfc"))
        assert np.abs(read_htk(WAV_PARM)[0] - read_htk(os.path.join(d, "plain.mfc"))[0]).max() > 1e-3
    write_npz(NPZ, arrs)
    with open(CONF, "w") as f:
        for case in sorted(CASES):
            f.write("[%s]\n%s\n" % (case, conf_text(case)))
    print("%d cases, %d bytes" % (len(CASES), os.path.getsize(NPZ)))
