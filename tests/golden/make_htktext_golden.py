"""Record what the reference's text routines make of a fixed set of inputs: tests/golden/htktext/htktext.json.

    make -C oracle _ref/ref_strings && python tests/golden/make_htktext_golden.py

Runs oracle/_ref/ref_strings (oracle/ref_strings.c) once per input, so that a refusal of the reference ends only that case.  The
JSON holds inputs and recorded outputs only; bytes are written as hex.  tests/test_htktext_host.py reads it and never the reference.
"""
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_strings")
OUT = os.path.join(ROOT, "tests", "golden", "htktext", "htktext.json")

# ---- ReadString: one text each (a newline inside is part of the text) ----
READ = [
    b"bare next\n", b"'single quoted' x\n", b'"double quoted" x\n', b'"it\'s" \'say "hi"\'\n',
    b"a\\\\b\n", b'a\\"b\n', b"a\\'b\n", b"a\\qb\n", b"oct\\351x\n", b"a\\8b\n", b"a\\12x rest\n", b"tail\\", b"tail\\\n",
    b'"open at end of line\nnext\n', b'"open at end of text', b'"" \'\' after\n', b"x'y \"z\n", b"\\\"lead \\'lead\n",
    b'"two words" -1.5\n', b"back\\\\slash\n", b"\\\"lead\n", b"oct\\351x\n",
    # the stop characters of ParseAlpha and GetAlpha, bare and quoted (ReadString itself stops at none of them)
    b"a.b a,b a)b a}b\n", b'"a.b" "a,b" "a)b" "a}b"\n',
    b"   \t  \n", b"",
    b"x" * 1500 + b"\n",
]
# ---- ReWriteString ----
WRITE = [b"plain", b"two words", b"'lead", b'"lead', b"mid'dle", b'mid"dle', b"back\\slash", b"\x01ctl", b"del\x7f", b"e\xe9", b"a.b,c)d}e",
         b"oct\xe9x", b"\\", b"'", b'"']
# ---- label files ----
LABELS = [
    b'0 100 "two words" -1.5\n100 200 back\\\\slash\n200 300 \\"lead\n300 400 oct\\351x\n',
    b"0 100 a -1.0\n100 200 'b c' -2.5 aux\n",
    b'0 100 "never closed\n',
]
# ---- dictionaries ----
LONG = b"LONG " + b" ".join(b"a_phone_with_a_long_name_%04d" % i for i in range(180)) + b"\n"      # > 4096 bytes, within MAXPHONES
DICTS = [
    b"A a b\nB [] b\nC [out] c\nD \"[two words]\" d\nE [two words] e\n",
    b"P1 1 a\nP2 0.5 a\nP3 .5 a\nP4 1e-7 a\nP5 [o] 0.25 a b\n",
    b"Q 1abc a\n",
    b"R 0.5 0.5 a\n",
    b"O [a] [b] x\n",
    b"oct\\351 a\\\\b 'q r'\n",
    LONG + b"AFTER a\n",
    b"U \"open\n",
    b"",
]


def run(mode, data, as_file=True):
    if as_file:
        with tempfile.NamedTemporaryFile(delete=False) as f:
            f.write(data)
        arg = f.name
    else:
        arg = data.hex()
    try:
        r = subprocess.run([REF, mode, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    finally:
        if as_file:
            os.unlink(arg)
    return {"in": data.hex(), "ok": r.returncode == 0, "out": r.stdout.decode().splitlines()}


def main():
    rec = {
        "about": "inputs (hex) and what oracle/ref_strings.c printed for them; ok = false: the reference refused (HError)",
        "read": [run("read", d) for d in READ],
        "write": [run("write", d, as_file=False) for d in WRITE],
        "labels": [run("labels", d) for d in LABELS],
        "dict": [run("dict", d) for d in DICTS],
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
