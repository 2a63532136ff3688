#!/usr/bin/env python3
"""Generate tests/golden/adpcm_decode_ref.npz from the REFERENCE's own libpsxav (oracle/_ref/libpsxav_ref.so, built unchanged by
oracle/Makefile): what its encoder reports while it encodes the decoder corpus (tests/adpcm_decode_corpus.py) -- after every SPU
unit (prev1, prev2, mse), after every XA sector the channel states.  Those are what a decoder plus a squared-error sum must
reproduce (libpsxav/adpcm.c:120-136).  The fixture holds these numbers and the corpus parameters, no input and no output bytes: the
signals are regenerated at test time.
Run where the reference build exists:  python tests/golden/make_adpcm_decode_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import adpcm_decode_corpus as DC  # noqa: E402
import oracle_lib as O  # noqa: E402


def main():
    assert O.ref() is not None, "oracle/_ref/libpsxav_ref.so missing: run make -C oracle with the reference tree present"
    out = {"meta": np.array([DC.SEED, DC.SPU_UNITS, DC.XA_SECTORS, DC.KINDS], np.int64)}
    for name in DC.signal_names():
        _, rep = DC.spu_encode_units(DC.signal(name, 28 * DC.SPU_UNITS), True)
        out["spu_" + name] = rep
        for fmt, stereo, bits in DC.XA_LAYOUTS:
            _, rep = DC.xa_encode_sectors(DC.xa_pcm(name, stereo, bits), fmt, stereo, bits, True)
            out[DC.xa_key(name, fmt, stereo, bits)] = rep
    np.savez_compressed(DC.GOLDEN, **out)
    print("wrote", DC.GOLDEN, "with", len(out), "arrays,", os.path.getsize(DC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
