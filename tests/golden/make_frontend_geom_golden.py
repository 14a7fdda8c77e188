#!/usr/bin/env python3
"""Golden vectors for the waveform front end away from 16 kHz / 25 ms: every FFT size from 8 to 4096 points, windows with no and with
almost all zero padding, sample periods that are no whole number of 100 ns units, the lane layouts on either side of the
two-frames-per-wavefront limits, and regression windows other than 2 / 2 on utterances shorter than the window.

Every case is a batch of a few short synthetic waveforms (case_waves: seeded, not committed) written as WAV files at the case's rate.
The configurations carry no SOURCERATE, so the reference takes the period from the WAV header (1e7 / rate as a double, HWave.c:1107).
The reference's HCopy (oracle/_ref, built from the reference tree by oracle/Makefile) codes each file alone; the rows of a batch, back
to back, and its frame offsets go into tests/golden/wave/frontend_geom.npz (<case> / <case>_off), the configuration texts into
tests/golden/wave/frontend_geom.conf (one "[case]" section each).

    make -C oracle _ref/HCopy && python tests/golden/make_frontend_geom_golden.py
"""
import os
import sys
import tempfile
import wave
import zipfile
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_frontend_golden import hcopy, read_htk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "wave")
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")
NPZ = os.path.join(OUT, "frontend_geom.npz")
CONF = os.path.join(OUT, "frontend_geom.conf")

COMMON = "SOURCEFORMAT = WAV\nPREEMCOEF = 0.97\nUSEHAMMING = T\n"
MFCC = "NUMCHANS = 26\nNUMCEPS = 12\nCEPLIFTER = 22\nENORMALISE = F\n"
PLP = "NUMCHANS = 26\nNUMCEPS = 12\nLPCORDER = 12\nUSEPOWER = T\nCEPLIFTER = 22\nENORMALISE = F\n"
BAND = "LOFREQ = 300\nHIFREQ = 3400\n"

# geometry row -> (rate in Hz, WINDOWSIZE, TARGETRATE, frSize, fftN)
GEOMS = {
    "g128": (8000, 100000.0, 100000.0, 80, 128),       # nn 64: stage pairs only, 16 work items for 64 lanes
    "g256": (8000, 250000.0, 100000.0, 200, 256),      # nn 128: a lone last stage
    "g512": (16000, 320000.0, 100000.0, 512, 512),     # no zero padding
    "g1024p": (16000, 320625.0, 100000.0, 513, 1024),  # a lone last stage, almost all padding
    "g1024": (22050, 250000.0, 100000.0, 551, 1024),   # period 453.51..
    "g2048": (48000, 250000.0, 100000.0, 1200, 2048),  # nn 1024, 10 stages; period 208.33..
    "g4096": (48000, 500000.0, 100000.0, 2400, 4096),  # the largest size: two frames do not fit one workgroup's LDS
    "g8": (16000, 5000.0, 2500.0, 8, 8),               # the smallest size
    "g512r": (44100, 100000.0, 100000.0, 441, 512),    # period 226.75..: 441 samples a frame and a shift only with the period as a double
    "std": (16000, 250000.0, 100000.0, 400, 512),      # the usual geometry, for the lane layouts and the regression windows
}
FRAMES = (1, 2, 7, 3)                                  # frames per utterance; an odd total: the last wavefront of a paired launch holds one frame
WIDE = (1, 2, 4)                                       # the same for the cases with many columns

# case -> (geometry row, TARGETKIND, the settings that matter, frames per utterance)
CASES = {}
for _g in GEOMS:
    if _g in ("std", "g512r"):
        continue
    small = _g == "g8"                                 # 3 FFT bins in the band: 3 channels, 2 cepstra
    CASES[_g + "_mfcc"] = (_g, "MFCC_0_D_A", "NUMCHANS = 3\nNUMCEPS = 2\nCEPLIFTER = 22\nENORMALISE = F\n" if small else MFCC, FRAMES)
    CASES[_g + "_fbank"] = (_g, "FBANK", "NUMCHANS = 3\n" if small else "NUMCHANS = 26\n", FRAMES)
for _g in ("g256", "g1024", "g4096"):
    CASES[_g + "_plp"] = (_g, "PLP_0_D_A", PLP, FRAMES)
    CASES[_g + "_melspec"] = (_g, "MELSPEC", "NUMCHANS = 26\n", FRAMES)
for _g in ("g1024", "g2048"):
    CASES[_g + "_mfcc_band"] = (_g, "MFCC_0_D_A", MFCC + BAND, FRAMES)
CASES.update({
    "g512r_mfcc": ("g512r", "MFCC_0_D_A", MFCC, FRAMES),
    # the limits of two frames per wavefront: 32 channels, 31 cepstra (C0 from lane 31), LPC order 31 -- and one beyond each
    "std_mfcc_c32_n31": ("std", "MFCC_0", "NUMCHANS = 32\nNUMCEPS = 31\nCEPLIFTER = 22\n", FRAMES),
    "std_mfcc_c33": ("std", "MFCC_0", "NUMCHANS = 33\nNUMCEPS = 12\nCEPLIFTER = 22\n", FRAMES),
    "std_mfcc_c40_n32": ("std", "MFCC_0", "NUMCHANS = 40\nNUMCEPS = 32\nCEPLIFTER = 22\n", FRAMES),
    "std_plp_c32_p31": ("std", "PLP_0", "NUMCHANS = 32\nNUMCEPS = 12\nLPCORDER = 31\nUSEPOWER = T\nCEPLIFTER = 22\n", FRAMES),
    "std_plp_p32": ("std", "PLP_0", "NUMCHANS = 26\nNUMCEPS = 12\nLPCORDER = 32\nUSEPOWER = T\nCEPLIFTER = 22\n", FRAMES),
    "std_plp_c40_p12": ("std", "PLP_0", "NUMCHANS = 40\nNUMCEPS = 12\nLPCORDER = 12\nUSEPOWER = T\nCEPLIFTER = 22\n", FRAMES),
    # more channels than lanes: the strided bin loops
    "std_fbank_c64": ("std", "FBANK", "NUMCHANS = 64\n", WIDE),
    "std_fbank_c65": ("std", "FBANK", "NUMCHANS = 65\n", WIDE),
    "std_fbank_c130": ("std", "FBANK", "NUMCHANS = 130\n", WIDE),
    "std_melspec_c65": ("std", "MELSPEC", "NUMCHANS = 65\n", WIDE),
    # regression windows 3 / 1 on utterances shorter than, as long as and longer than the window
    "std_mfcc_win31": ("std", "MFCC_E_D_A_Z", "NUMCHANS = 26\nNUMCEPS = 12\nCEPLIFTER = 22\nENORMALISE = T\nDELTAWINDOW = 3\nACCWINDOW = 1\n",
                       (1, 2, 3, 7, 40)),
})


def rate(case):
    return GEOMS[CASES[case][0]][0]


def conf_text(case):
    geom, kind, extra, _ = CASES[case]
    _, win, tgt, _, _ = GEOMS[geom]
    return COMMON + "WINDOWSIZE = %.1f\nTARGETRATE = %.1f\nTARGETKIND = %s\n" % (win, tgt, kind) + extra


def case_waves(case):
    """The case's batch: sine plus noise at the case's rate, int16, each utterance a few samples longer than its frames need."""
    geom, _, _, frames = CASES[case]
    hz, _, _, frSize, _ = GEOMS[geom]
    frRate = int(GEOMS[geom][2] / (1.0e7 / hz))
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    out = []
    for i, nf in enumerate(frames):
        n = frSize + (nf - 1) * frRate + int(rng.integers(0, frRate))
        t = np.arange(n) / float(hz)
        x = 2500 * np.sin(2 * np.pi * (300 + 170 * i) * t) + 1200 * np.sin(2 * np.pi * 2100 * t) + rng.normal(0, 600 + 100 * i, n)
        out.append(x.clip(-32768, 32767).astype("<i2"))
    return out


def write_wav(path, x, hz):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(hz); w.writeframes(np.asarray(x, "<i2").tobytes())


def code_batch(exe, case, waves, d):
    """HCopy on every wave of `waves` with case `case`'s configuration: the rows of all of them, back to back, and the frame offsets."""
    conf = os.path.join(d, "%s.conf" % case)
    open(conf, "w").write(conf_text(case))
    rows, off = [], [0]
    for i, x in enumerate(waves):
        src, dst = os.path.join(d, "%s_%d.wav" % (case, i)), os.path.join(d, "%s_%d.htk" % (case, i))
        write_wav(src, x, rate(case))
        hcopy(exe, conf, src, dst)
        r, _ = read_htk(dst)
        rows.append(r); off.append(off[-1] + r.shape[0])
    return np.concatenate(rows), np.asarray(off, np.int32)


def read_confs(path=CONF):
    """The committed configuration texts: case -> text."""
    out, cur = {}, None
    for line in open(path):
        if line.startswith("["):
            cur = line.strip()[1:-1]; out[cur] = ""
        elif cur is not None and line.strip():
            out[cur] += line
    return out


def write_npz(path, arrs):
    """np.savez_compressed with the members' timestamps fixed: the same rows give the same bytes."""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    if not os.path.exists(HCOPY):
        sys.exit("needs %s (make -C oracle _ref/HCopy)" % HCOPY)
    arrs = {}
    with tempfile.TemporaryDirectory() as d:
        for case in sorted(CASES):
            rows, off = code_batch(HCOPY, case, case_waves(case), d)
            geom, kind, _, frames = CASES[case]
            assert list(np.diff(off)) == list(frames), (case, off, frames)
            arrs[case] = rows; arrs[case + "_off"] = off
            print(case, kind, rows.shape, list(off))
    write_npz(NPZ, arrs)
    with open(CONF, "w") as f:
        for case in sorted(CASES):
            f.write("[%s]\n%s\n" % (case, conf_text(case)))
    print("%d cases, %d bytes" % (len(CASES), os.path.getsize(NPZ)))
