"""Damaged sectors for the disc reader's tests (tests/test_disc_read_ref.py, tests/test_gpu_disc_read.py): finished images from the
statement of the finisher (tests/disc_ref.py) and every damage class "psxhip disc read v1"  speaks of."""
import numpy as np

import disc_ref as R

SINGLE_BYTES = (0x10, 0x12, 0x17, 0x18, 0x817, 0x818, 0x81B, 0x81C, 0x8C7, 0x8C8, 0x92F)
BURSTS = tuple((n, at) for n in (2, 43, 86, 87) for at in (0x18, 0x123, 0x700))
LONG_BURSTS = (172, 300, 600)


def sectors(rng, n, size, pad=0, forms=None, kind=0x08):
    """n random sectors of `size` bytes in rows of size + pad whose submode has the bit `kind` (0x08 data, 0x04 audio, 0x02 video) and
    none of the other two; forms: per sector 1 / 2 (None: 1), ignored by 2048-byte sources"""
    data = rng.integers(0, 256, (n, size + pad)).astype(np.uint8)
    at = {2352: 0x12, 2336: 2}.get(size)
    if at is not None:
        data[:, at] = (data[:, at] & 0xD1) | kind
        for k in range(n):
            if forms is not None and forms[k] == 2:
                data[k, at] |= 0x20
    return data


def form1_image(rng, n, start_lba=0, file=1, channel=0):
    """n finished random form-1 sectors"""
    return R.finish([0], start_lba, [R.Source(sectors(rng, n, 2336), 2336, file=file, channel=channel)])


def flip(sector, places, rng):
    """a copy of the sector with every byte of `places` wrong"""
    bad = sector.copy()
    for at in places:
        bad[at] ^= rng.integers(1, 256)
    return bad


def burst(sector, n, at, rng):
    return flip(sector, range(at, at + n), rng)


def scattered(sector, n, rng):
    """n wrong bytes at random places of 0x10 .. 0x92F"""
    return flip(sector, rng.choice(np.arange(0x10, 0x930), n, replace=False), rng)


def one_bad_column(sector, rng):
    """damage inside 0x10 .. 0x8C7 in which at most one P column holds more than one wrong byte: what the statement always repairs"""
    cols = rng.permutation(86)
    many, singles = int(cols[0]), cols[1:1 + rng.integers(0, 41)]
    rows = rng.choice(26, rng.integers(2, 25), replace=False)
    places = [12 + many + 86 * int(i) for i in rows] + [12 + int(m) + 86 * int(rng.integers(0, 26)) for m in singles]
    return flip(sector, [at for at in places if at >= 0x10], rng)


def damage_classes(rng, clean):
    """(name, damaged sector, original, repairable) for every class; `clean` supplies finished form-1 sectors in turn"""
    out = []
    it = iter(clean)
    for at in SINGLE_BYTES:
        s = next(it)
        out.append(("byte 0x%X" % at, flip(s, [at], rng), s, True))
    for n, at in BURSTS:
        s = next(it)
        out.append(("burst %d at 0x%X" % (n, at), burst(s, n, at, rng), s, True))
    for n in (2, 3, 5, 8, 13, 21, 32):
        s = next(it)
        out.append(("%d scattered" % n, scattered(s, n, rng), s, True))
    for n in LONG_BURSTS:
        s = next(it)
        out.append(("burst %d" % n, burst(s, n, 0x200, rng), s, False))
    return out


N_DAMAGE_CLASSES = len(SINGLE_BYTES) + len(BURSTS) + 7 + len(LONG_BURSTS)
