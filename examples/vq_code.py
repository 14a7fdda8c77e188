"""HCopy with a _V target kind, VQTABLE and SAVEASVQ: parameter files coded into DISCRETE files on the device.

    python examples/vq_code.py vqFile src1 tgt1 [src2 tgt2 ...]

All the files are coded in one call (htkamd_vq_code); the table's streams are consecutive column ranges of the data.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi  # noqa: E402


def main(argv):
    if len(argv) < 3 or len(argv) % 2 == 0:
        raise SystemExit(__doc__)
    tab = capi.VQ(path=argv[0])
    pairs = list(zip(argv[1::2], argv[2::2]))
    data = [capi.parm_read(src) for src, _ in pairs]
    for (src, _), (X, _, kind) in zip(pairs, data):
        if tab.magic != kind:
            raise SystemExit("LoadVQTab: %s has magic=%d but %s is of kind %d" % (argv[0], tab.magic, src, kind))
    off = capi.offsets([len(X) for X, _, _ in data])
    dX = capi.DevArray(np.concatenate([X for X, _, _ in data]))
    codes = tab.code(dX.ptr, off, data[0][0].shape[1])
    dX.free()
    for u, ((_, tgt), (_, per, _)) in enumerate(zip(pairs, data)):
        capi.parm_write_discrete(tgt, codes[off[u]:off[u + 1]], per, withCrc=True)      # (HCopy's default: SAVEWITHCRC)
    return codes


if __name__ == "__main__":
    main(sys.argv[1:])
