"""A model of the split kernel's rendezvous (csrc/mdec_split.inc), run under random interleavings.

The GPU tests check bytes; they cannot choose the schedule.  Here every workgroup of one frame is a little state machine that performs
ONE shared-memory operation per step on the same words as the kernel -- its v3 DC words, its slots per round of scales, the other
groups' words read until they are there, image ORs, its done word; the finisher's wait for the done words and its zeroing of the
workspace; since the release fix the exit count and the last group's clean-up -- and a seeded scheduler picks who moves next.  Groups
start late (not resident), and a wait gives up after a seeded number of looks (the watchdog).  Launches follow each other on ONE
workspace with the segment counts psxhip_mdec_split_geometry picks for 1..12 frames, and the next launch starts when every group of
the one before has left (split launches of a device are serialised).

Every published word carries the launch that wrote it, so a read of another launch's word is seen.  Properties: each launch ends
with the first-fit answer and its exact image, or "released"; no group ever takes a word of an earlier launch; the workspace is all
zero when the last group leaves.  Under the old rules (the finisher alone zeroes the workspace, once, whatever comes after it) some
schedule lets a later launch take a stale word; under the new ones none of 20 000 schedules does."""
import random

import pytest

ROUND = 4           # scales per round
ROUNDS = 3          # scales 1 .. 12
NMB = 12            # macroblocks of the frame
N_CU = 8            # compute units of the modelled device
IMG = 1024          # image words


def geometry(n_frames):
    """psxhip_mdec_split_geometry: M doubles from 2 until segments x frames fit the CUs"""
    m = 2
    while m < 16 and -(-NMB // m) * n_frames > N_CU:
        m *= 2
    return m, -(-NMB // m)


class Frame:
    """content: DC terms and the bits of every macroblock at every scale (the DC deltas add to them: a wrong DC word, a wrong sum)"""

    def __init__(self, rng):
        self.dc = [rng.randint(1, 1023) for _ in range(NMB)]
        self.base = [rng.randint(20, 90) for _ in range(NMB)]
        self.limit = rng.randint(250, 700)

    def bits(self, mb, scale, dc):
        delta = abs(dc[mb] - (dc[mb - 1] if mb else 512))
        return self.base[mb] * 4 // (scale + 3) + delta.bit_length()

    def code(self, mb, scale, dc):
        return (hash((mb, scale, dc[mb], self.base[mb])) & 0xFFFF) | 1

    def expected(self):
        """(answer, image) of the reference's ascending scan, or (64, None)"""
        for s in range(1, ROUND * ROUNDS + 1):
            img = {}
            at = 0
            for mb in range(NMB):
                img[at] = self.code(mb, s, self.dc)
                at += self.bits(mb, s, self.dc)
            if at <= self.limit:
                return s, img
        return 64, None


class Workspace:
    """words are None (zero) or (launch, value); image words are (launches, OR of values)"""

    def __init__(self):
        self.slots = [None] * (ROUNDS * NMB)          # [round][segment]: the segment's sums of the round's scales
        self.dcw = [None] * NMB
        self.img = [None] * IMG
        self.done = [None] * NMB
        self.exits = 0                                # groups out | 0x10000: released

    def clean(self):
        return (all(v is None for v in self.slots + self.dcw + self.img + self.done) and self.exits == 0)


class Launch:
    def __init__(self, lid, frame, n_frames):
        self.lid, self.frame = lid, frame
        self.M, self.segs = geometry(n_frames)
        self.result = None
        self.stale = []                               # (group, what) for every word of another launch a group took


def group(ws, L, g, rng, patience, delay, new_rules):
    """generator: one yield per shared-memory operation"""
    F, M, segs = L.frame, L.M, L.segs
    mbs = range(g * M, min(NMB, (g + 1) * M))
    for _ in range(delay):
        yield

    def take(word, what):
        if word[0] != L.lid if isinstance(word[0], int) else any(x != L.lid for x in word[0]):
            L.stale.append((g, what))
        return word[1]

    def await_(get, what):
        """looks at a word until it is there or patience runs out (the watchdog): returns its value or None"""
        for _ in range(patience + 1):
            w = get()
            yield
            if w is not None:
                return take(w, what)
        return None

    # phase A: the segment's DC terms for everybody, then every DC term
    for mb in mbs:
        ws.dcw[mb] = (L.lid, F.dc[mb])
        yield
    alive, dc = True, [0] * NMB
    for mb in range(NMB):
        v = yield from await_(lambda mb=mb: ws.dcw[mb], "dc")
        if v is None:
            alive = False
            break
        dc[mb] = v
    # phase B: rounds of scales
    answer, tot_at, pre_at, rounds_used = 0, None, None, 0
    r = 0
    while alive and r < ROUNDS:
        rounds_used = r + 1
        scales = range(r * ROUND + 1, (r + 1) * ROUND + 1)
        mine = tuple(sum(F.bits(mb, s, dc) for mb in mbs) for s in scales)
        ws.slots[r * NMB + g] = (L.lid, mine)
        yield
        sums = []
        for h in range(segs):
            v = yield from await_(lambda h=h: ws.slots[r * NMB + h], "slot")
            if v is None:
                alive = False
                break
            sums.append(v)
        if not alive:
            break
        for k, s in enumerate(scales):
            tot = sum(x[k] for x in sums)
            if tot <= F.limit:
                answer, pre_at = s, sum(x[k] for x in sums[:g])
                break
        if answer:
            break
        r += 1
    # phase C: the segment's codes ORed into the image at their place
    if alive and answer:
        at = pre_at
        for mb in mbs:
            if at < IMG:
                old = ws.img[at]
                ws.img[at] = ((old[0] if old else frozenset()) | {L.lid}, (old[1] if old else 0) | F.code(mb, answer, dc))
                yield
            at += F.bits(mb, answer, dc)
    ws.done[g] = (L.lid, 1 if alive else 2)
    yield
    tripped = False
    if g == segs - 1:
        # the finisher: every done word, the frame's row, then the workspace back to zero
        for h in range(segs):
            v = yield from await_(lambda h=h: ws.done[h], "done")
            tripped = tripped or v != 1
        if tripped or not answer:
            L.result = ("released",) if tripped else (64, None)
        else:
            img = {}
            for i in range(IMG):
                w = ws.img[i]
                if w is not None:
                    img[i] = take(w, "image")
            L.result = (answer, img)
            yield
        for i in range(0, IMG, 128):
            for j in range(i, i + 128):
                ws.img[j] = None
            yield
        for rr in range(rounds_used):
            for h in range(segs):
                ws.slots[rr * NMB + h] = None
            yield
        for mb in range(NMB):
            ws.dcw[mb] = None
        yield
        for h in range(segs):
            ws.done[h] = None
        yield
    if new_rules:
        # leaving: the count, and the last one out of a released frame returns the workspace to zero
        ws.exits += 0x10001 if tripped else 1
        now = ws.exits
        yield
        if now & 0xFFFF == segs:
            if now >> 16:
                ws.img = [None] * IMG
                yield
                for rr in range(ROUNDS):
                    for h in range(segs):
                        ws.slots[rr * NMB + h] = None
                    yield
                ws.dcw = [None] * NMB
                ws.done[:segs] = [None] * segs
                yield
            ws.exits = 0
            yield


def run_schedule(seed, new_rules):
    rng = random.Random(seed)
    ws = Workspace()
    launches = []
    for lid in range(4):
        n = rng.choice((1, 1, 2, 3, 12))
        L = Launch(lid, Frame(rng), n)
        launches.append(L)
        kind = rng.random()
        gens = []
        for g in range(L.segs):
            late = rng.random() < (0.3 if kind < 0.5 else 0.05)
            delay = rng.randint(0, 150) if late else rng.randint(0, 3)
            patience = rng.choice((0, 1, 3, 10, 40, 200))
            gens.append(group(ws, L, g, rng, patience, delay, new_rules))
        while gens:
            k = rng.randrange(len(gens))
            try:
                next(gens[k])
            except StopIteration:
                gens.pop(k)
    return ws, launches


def check(ws, launches):
    """the properties; returns a list of what went wrong"""
    bad = []
    for L in launches:
        if L.stale:
            bad.append("launch %d took words of an earlier launch: %s" % (L.lid, L.stale[:3]))
        want = L.frame.expected()
        if L.result is None:
            bad.append("launch %d: no result" % L.lid)
        elif L.result != ("released",) and L.result != want:
            bad.append("launch %d: wrong result (answer %s, want %s)" % (L.lid, L.result[0], want[0]))
    if not ws.clean():
        bad.append("workspace not zero after the last launch")
    return bad


def test_geometry_matches_the_host():
    assert [geometry(n) for n in (1, 2, 3, 12)] == [(2, 6), (4, 3), (8, 2), (16, 1)]


def test_without_any_release_every_launch_is_exact():
    """patient, resident groups: the reference's answer and image, every time, under both rule sets"""
    for new_rules in (False, True):
        for seed in range(50):
            rng = random.Random(seed)
            ws = Workspace()
            launches = []
            for lid, n in enumerate((1, 12, 3, 1)):
                L = Launch(lid, Frame(rng), n)
                launches.append(L)
                gens = [group(ws, L, g, rng, 10 ** 6, 0, new_rules) for g in range(L.segs)]
                while gens:
                    k = rng.randrange(len(gens))
                    try:
                        next(gens[k])
                    except StopIteration:
                        gens.pop(k)
            assert check(ws, launches) == [], seed
            assert all(L.result != ("released",) for L in launches)


def test_old_rules_let_a_later_launch_take_a_stale_word():
    """the finisher alone zeroing the workspace: a late group of a released frame publishes after it, and the next launch reads that
    as its own arrival -- the model finds such a schedule"""
    found = None
    for seed in range(2000):
        ws, launches = run_schedule(seed, new_rules=False)
        bad = check(ws, launches)
        if any("earlier launch" in b for b in bad):
            found = (seed, bad)
            break
    assert found is not None, "the model no longer sees the defect it was written for"


def test_new_rules_hold_over_20000_schedules():
    releases = 0
    for seed in range(20000):
        ws, launches = run_schedule(seed, new_rules=True)
        bad = check(ws, launches)
        assert bad == [], (seed, bad)
        releases += sum(L.result == ("released",) for L in launches)
    assert releases > 1000, releases          # (the schedules do release frames: the path is exercised)
