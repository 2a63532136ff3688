#!/usr/bin/env python3
"""Generate tests/golden/adpcm_chain_corpus_ref.npz from the REFERENCE's own libpsxav (oracle/_ref/libpsxav_ref.so, built unchanged by
oracle/Makefile): what it makes of the cases of the encoder's chain corpus (tests/adpcm_encode_corpus.py) that it can express --
every SPU case through psx_audio_spu_encode at the chain's pitch, the XA streams through psx_audio_xa_encode in every XA layout.
Per case the fixture holds one SHA-256 over the reference's bytes and end states, and the corpus parameters; no input, no output.
Run where the reference build exists:  python tests/golden/make_adpcm_chain_corpus_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import adpcm_encode_corpus as EC  # noqa: E402
import oracle_lib as O  # noqa: E402


def build():
    assert O.ref() is not None, "oracle/_ref/libpsxav_ref.so missing: run make -C oracle with the reference tree present"
    out = {"meta": np.array([EC.SEED, EC.MAX_CHAINS, EC.MAX_UNITS, EC.N_KINDS, EC.XA_SECTORS], np.int64)}
    for name in EC.LAYOUTS:
        for n_chains in EC.CHAIN_COUNTS:
            out[EC.spu_key(name, n_chains)] = EC.digest(*EC.spu_reference(name, n_chains))
    for fmt, stereo, bits in EC.XA_LAYOUTS:
        sectors, final = EC.xa_sectors(fmt, stereo, bits, True)
        out[EC.xa_key(fmt, stereo, bits)] = EC.digest(EC.xa_group_bytes(sectors, fmt), final)
    return out


def main():
    out = build()
    np.savez_compressed(EC.GOLDEN, **out)
    print("wrote", EC.GOLDEN, "with", len(out), "arrays,", os.path.getsize(EC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
