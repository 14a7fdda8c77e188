"""The tree-clustering fixture (tests/golden/treeclust, made by tests/golden/make_treeclust_golden.py) as files: the model sets are
committed gzip-compressed, and the HMM list is the models' names in the order of their definitions."""
import gzip
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "treeclust")


def golden_bytes(name: str) -> bytes:
    """A committed file of the fixture, unpacked where it is stored as name.gz."""
    p = os.path.join(G, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    return gzip.open(p + ".gz", "rb").read()


def unpack_inputs(workdir) -> tuple:
    """hmmdefs and hmmlist under workdir; returns their paths."""
    mmf, lst = os.path.join(str(workdir), "hmmdefs"), os.path.join(str(workdir), "hmmlist")
    text = golden_bytes("hmmdefs")
    with open(mmf, "wb") as f:
        f.write(text)
    with open(lst, "w") as f:
        f.write("\n".join(re.findall(r'^~h "([^"]+)"', text.decode(), flags=re.M)) + "\n")
    return mmf, lst
