""""psxhip SPU loop seam v1"  in plain Python: the statement the seam tables of the plan
(psxavenc_amd/csrc/spu_bank_plan.cpp), the step and the report (psxavenc_amd/csrc/spu_seam_core.h, spu_seam_kernels.hip) and
mode STEADY of psxhip_spu_bank_encode_device are held to.  It rests on the reference's SPU encoder with a carried state (the
reference build's psx_audio_spu_encode where it is there, else oracle/adpcm_oracle.c, which tests/test_adpcm_oracle.py holds to it),
on tests/adpcm_beam_ref.py for a beam of 2 .. 4 and on tests/adpcm_decode_ref.py.

A looped sample plays intro, body, body, ...  The encoder plans the loop-start block from the state the intro leaves; on every repeat
the SPU enters it with the state the END of the body left.  Entries are the dicts of tests/spu_bank_corpus.py."""
import numpy as np

import adpcm_beam_ref as BR
import adpcm_decode_ref as R
import oracle_lib as O

PASSES = 8
OFF, STEADY = 0, 1


def data_blocks(e):
    return -(-e["samples"] // 28)


def seam_block(s, e):
    """the seam block S of an entry, or -1"""
    D = data_blocks(e)
    if not e["enable_loop"] or D == 0:
        return -1
    start = e["loop"] * e["freq"] // 28000 if e["loop"] >= 0 else -1
    if 0 <= start < D:
        return start                            # the block that carries LOOP_START
    return 0 if s["no_dummy"] else -1           # key-on sets the repeat address to the start address: block 0, or the dummy block


def padded(e, pcm):
    """the entry's PCM over its whole units, zero past `samples`"""
    x = np.zeros(28 * data_blocks(e), np.int16)
    x[:e["samples"]] = pcm[e["pcm_offset"]:e["pcm_offset"] + e["samples"]]
    return x


def encode_chains(xs, states, beam):
    """the bank's encoder over whole units: xs a list of int16 arrays (multiples of 28 samples), states a list of (prev1, prev2)
    -> [(blocks (units, 16) uint8 with byte 1 zero, (prev1, prev2) behind the last unit)]"""
    out = []
    if beam < 2:
        for x, st in zip(xs, states):
            if O.ref() is not None:
                blocks, end = O.ref_spu_encode(x, state=O.RefChan(0, 0, int(st[0]), int(st[1])))
            else:
                blocks, end = O.spu_encode(x, state=O.Chan(int(st[0]), int(st[1])))
            out.append((blocks.reshape(-1, 16).copy(), (int(end.prev1), int(end.prev2))))
        return out
    if not xs:
        return out
    units = np.array([len(x) // 28 for x in xs])
    m = np.zeros((len(xs), 28 * int(units.max())), np.int16)
    for i, x in enumerate(xs):
        m[i, :len(x)] = x
    rec, _, after, _ = BR.encode_chains_np(m, np.array(states, np.int64).reshape(-1, 2), units, 5, 4, beam)
    for i, n in enumerate(units):
        out.append((rec[i, :n].copy(), (int(after[i, n - 1, 0]), int(after[i, n - 1, 1])) if n else tuple(states[i])))
    return out


def encode_entries(xs, seams, beam, mode, trace=None):
    """the data blocks of a bank's entries, byte 1 zero.  xs: per entry its padded PCM; seams: per entry S or -1
    -> ([blocks (D, 16)], [outcome]): outcome -1 without a seam block, k = fixed at pass k, PASSES = pass 0 kept; under mode OFF
    every entry is one chain from a zero state and the outcomes are None.  trace (a list): gets s_0 per looping entry, then per pass
    {entry: (s_k, e_k)} of the entries that pass encoded"""
    n = len(xs)
    if mode == OFF:
        return [b for b, _ in encode_chains(xs, [(0, 0)] * n, beam)], None
    # what is encoded once from a zero state: the intros and the entries without a seam block
    first = [i for i in range(n) if seams[i] != 0]
    got = encode_chains([xs[i] if seams[i] < 0 else xs[i][:28 * seams[i]] for i in first], [(0, 0)] * len(first), beam)
    head, s0 = {i: g[0] for i, g in zip(first, got)}, {i: g[1] for i, g in zip(first, got)}
    blocks, outcome = [None] * n, [-1] * n
    for i in first:
        if seams[i] < 0:
            blocks[i] = head[i]
    active = [i for i in range(n) if seams[i] >= 0]
    start = {i: s0.get(i, (0, 0)) for i in active}
    pass0 = {}
    if trace is not None:
        trace.append(dict(start))
    for k in range(PASSES):
        got = encode_chains([xs[i][28 * seams[i]:] for i in active], [start[i] for i in active], beam)
        still = []
        if trace is not None:
            trace.append({i: (start[i], end) for i, (_, end) in zip(active, got)})
        for i, (body, end) in zip(active, got):
            if k == 0:
                pass0[i] = body
            if end == start[i]:
                blocks[i], outcome[i] = body, k
            else:
                start[i] = end
                still.append(i)
        active = still
    for i in active:
        blocks[i], outcome[i] = pass0[i], PASSES
    for i in range(n):
        if seams[i] > 0:
            blocks[i] = np.concatenate([head[i], blocks[i]])
    return blocks, outcome


# ---- the report
FIELDS = ("seam_block", "first_units", "first_peak", "settled", "first_sse", "pass1_err", "pass2_err")


def report(blocks, S, x=None):
    """the statement: two whole decodes.  blocks (D, 16); S the seam block or -1; x the padded PCM or None"""
    out = dict.fromkeys(FIELDS, 0)
    out["seam_block"] = S
    if S < 0:
        return out
    blocks = np.asarray(blocks, np.uint8).reshape(-1, 16)
    D = len(blocks)
    p1, p2, before1 = 0, 0, []
    y1 = np.zeros(28 * D, np.int64)
    for u in range(D):
        before1.append((p1, p2))
        y1[28 * u:28 * u + 28], p1, p2, _ = R.decode_unit(blocks[u], 4, 5, p1, p2)
    b = (p1, p2)
    before2 = []
    y2 = np.zeros(28 * (D - S), np.int64)
    for u in range(S, D):
        before2.append((p1, p2))
        y2[28 * (u - S):28 * (u - S) + 28], p1, p2, _ = R.decode_unit(blocks[u], 4, 5, p1, p2)
    y1 = y1[28 * S:]
    out["first_units"] = next((k for k in range(D - S) if before1[S + k] == before2[k]), D - S)
    out["first_peak"] = int(np.abs(y2 - y1).max())
    out["first_sse"] = int(((y2 - y1) ** 2).sum())
    out["settled"] = int((p1, p2) == b)
    if x is not None:
        xb = np.asarray(x, np.int64)[28 * S:]
        out["pass1_err"], out["pass2_err"] = int(((y1 - xb) ** 2).sum()), int(((y2 - xb) ** 2).sum())
    return out


def report_early(blocks, S, x=None):
    """the report as the kernel computes it (spu_seam_core.h): pass 1 once, then pass 2 beside pass 1 until their states coincide"""
    out = dict.fromkeys(FIELDS, 0)
    out["seam_block"] = S
    if S < 0:
        return out
    blocks = np.asarray(blocks, np.uint8).reshape(-1, 16)
    D = len(blocks)
    xx = None if x is None else np.asarray(x, np.int64)
    a, at, err1 = (0, 0), (0, 0), 0
    for u in range(D):
        if u == S:
            at = a
        y, p1, p2, _ = R.decode_unit(blocks[u], 4, 5, *a)
        a = (p1, p2)
        if xx is not None and u >= S:
            err1 += int(((y - xx[28 * u:28 * u + 28]) ** 2).sum())
    b, k, peak, sse, delta = a, 0, 0, 0, 0
    while k < D - S and at != b:
        y1, p1, p2, _ = R.decode_unit(blocks[S + k], 4, 5, *at)
        at = (p1, p2)
        y2, p1, p2, _ = R.decode_unit(blocks[S + k], 4, 5, *b)
        b = (p1, p2)
        peak, sse = max(peak, int(np.abs(y2 - y1).max())), sse + int(((y2 - y1) ** 2).sum())
        if xx is not None:
            xs = xx[28 * (S + k):28 * (S + k) + 28]
            delta += int(((y2 - xs) ** 2).sum()) - int(((y1 - xs) ** 2).sum())
        k += 1
    out.update(first_units=k, first_peak=peak, first_sse=sse, settled=int(at == b), pass1_err=err1, pass2_err=err1 + delta)
    return out


# ---- the plan's seam tables, restated (p: the restated plan of tests/spu_bank_corpus.py)
def seam_tables(s, entries, p):
    """-> dict: seams [n]; chains [(sample_offset, pitch, sample_limit, n_units, unit_stride, unit_base)]: first, in entry order, the
    intro of every entry with S > 0 and the whole chain of every entry without a seam block, then, in entry order, the body of every
    entry with one; first / body their counts; bodies [(entry, the intro's slot or -1)]"""
    seams = [seam_block(s, e) for e in entries]

    def part(e, base, first, count):
        return (e["pcm_offset"] + 28 * first, 1, max(e["samples"] - 28 * first, 0), count, 1, base + first)
    chains, slot = [], {}
    for i, (e, S, base) in enumerate(zip(entries, seams, p["unit_base"])):
        if S != 0:
            slot[i] = len(chains)
            chains.append(part(e, base, 0, data_blocks(e) if S < 0 else S))
    first, bodies = len(chains), []
    for i, (e, S, base) in enumerate(zip(entries, seams, p["unit_base"])):
        if S >= 0:
            chains.append(part(e, base, S, data_blocks(e) - S))
            bodies.append((i, slot[i] if S > 0 else -1))
    return dict(seams=seams, chains=chains, first=first, body=len(bodies), bodies=bodies)
