"""What the input-transform tests and the fixture generator share: the NumPy float32 restatement of ApplyStaticMat's loop
(HTKLib/HParm.c:1266-1274), and the reader of a transform file's text form."""
import numpy as np


def xform_ref(M, X):
    """Row r of the result is M . X[r][0..mcols) as the reference computes it: every output starts at 0.0f, then for m = 0 .. mcols-1
    acc = acc + (M[j][m] * x[m]), the product and the sum each rounded to float32 (NumPy's float32 arithmetic rounds every operation
    to nearest and keeps subnormals)."""
    M = np.asarray(M, np.float32); X = np.asarray(X, np.float32)
    acc = np.zeros((X.shape[0], M.shape[0]), np.float32)
    for m in range(M.shape[1]):
        acc = acc + M[None, :, m] * X[:, m, None]
    assert acc.dtype == np.float32
    return acc


def macro_form(inline, name="proj20"):
    """A set with its transform inline behind the options, as the reference writes it (str: the text form; bytes: the binary form, whose
    <INPUTXFORM> keyword is ':' + code 109) -> (the transform as a ~j macro definition, the set with <INPUTXFORM> ~j "name" in its place).
    The two in one file are the macro form of the set; apart, the first is a transform file and the second names it."""
    binary = isinstance(inline, bytes)
    key, h, nl = (b":m", b'~h "', b"") if binary else ("<INPUTXFORM>", '~h "', "\n")
    ref = '~j "%s"' % name
    ref = (ref.encode() if binary else ref) + nl
    at = inline.index(key, inline.index(b"<DIAGC>" if binary else "<DIAGC>"))
    body = inline[at + len(key):inline.index(h)]
    return ref + body, inline[:at + len(key)] + (b"" if binary else " ") + ref + inline[inline.index(h):]


def wav_case_set(fitted_text, transform_text):
    """tests/golden/wave/fitted.mmf (39 dimensions, MFCC_0_D_A, fitted to test.wav) with an input transform behind its global options"""
    key = "<MFCC_0_D_A><DIAGC>\n"
    return fitted_text.replace(key, key + "<INPUTXFORM>" + transform_text, 1)


def with_kind(src, dst, old="<MFCC_E_D_A>", new="<MFCC_E_D_A_Z>"):
    """a transform file, text or binary, under another parameter kind (the kind is text in both forms)"""
    open(dst, "wb").write(open(src, "rb").read().replace(old.encode(), new.encode()))
    return dst


def read_xform_text(path):
    """A text transform (a file of its own, or the transform inside a text model file) -> dict(name, mask, kind, prequal, matrix)."""
    tok = open(path).read().split()
    i = tok.index("<MMFIDMASK>")
    out = {"name": tok[i - 1].strip('"') if i >= 2 and tok[i - 2] == "~j" else None, "mask": tok[i + 1]}
    head = tok[i + 2]
    out["prequal"] = "<PREQUAL>" in head
    out["kind"] = head.replace("<PREQUAL>", "").strip("<>")
    j = tok.index("<XFORM>", i)
    r, c = int(tok[j + 1]), int(tok[j + 2])
    out["matrix"] = np.array([np.float32(t) for t in tok[j + 3:j + 3 + r * c]], np.float32).reshape(r, c)
    return out
