"""Bit-level Python models of the two lane coders, and a generator of the lanes that random data never produces.

CarryCoder      container version 4: the carry-propagating coder (oracle/gpcc_oracle.c: cp_encode_core).  Every carry is
                recorded: how many one bits it flipped, and how many bits the string held when it arrived (modulo 32 that is
                the device writer's accumulator fill, BitOut::n; divided by 32 the words it has stored).
CarrylessCoder  torchac's coder (rc_encode_core: the reference layout and container versions 1-3).  Every resolution of the
                pending (underflow) count is recorded: the count, the bit, the agreed leading bits n1 that leave with it.

make_lane() steers a coder across a carry boundary.  The carry coder's interval [low, low + range) is kept astride
B = 2^31 (the first shift emits a 0 and moves B to 2^32) and narrowed from either side, so that the string grows by
0111...1; the last step either lifts `low` past B (one carry through the whole run), stops below it (the run stays), or the
lane ends there (the flush decides).  The carry-less coder's [low, high] is kept astride the midpoint the same way, which
grows `pending`; the last step resolves it to 0 or to 1.  Every step is chosen by running the model on a list of candidate
slices, never by trusting a formula: what the generator promises (run length, offsets, n1) is read back from the model.

Rows are full uint16 CDF rows as the codec holds them: row[0] = 0, row[1 .. Lp-2] strictly ascending in [1, 65535],
row[Lp-1] = 0 (65536 in 16 bits; never read)."""
from collections import namedtuple

import numpy as np

M32 = 0xFFFFFFFF
MID = 1 << 31

Carry = namedtuple("Carry", "flipped pos words flush")            # pos = bits held modulo 32, words = bits held // 32
Resolution = namedtuple("Resolution", "pending bit n1 pos flush")  # pos = bits written before it, modulo 32


def end_word(c):
    """Where a carry's ripple ends in the device writer: 0 = inside the accumulator, j >= 1 = in the j-th stored word
    counted back from the last one (j - 1 words wrapped to zero on the way)."""
    return 0 if c.flipped < c.pos else (c.flipped - c.pos) // 32 + 1


def _clz32(v):
    return 32 - v.bit_length() if v else 31    # (clz32c: 31 for 0)


def _trailing_ones(v):
    return ((~v) & (v + 1)).bit_length() - 1


def _bytes_of(val, nbits):
    pad = -nbits % 8
    return (val << pad).to_bytes((nbits + pad) // 8, "big")


def _slice_of(row, s):
    """(c_lo, c_hi) of symbol s; c_hi = None for the last symbol (65536: the coders take their `last symbol` branch)"""
    return int(row[s]), (None if s == len(row) - 2 else int(row[s + 1]))


# ------------------------------------------------------------------------------------------------ version 4
def cp_step(low, rng, c_lo, c_hi):
    """One symbol of cp_encode_core on (low, range): (carry, low before the shift, range before the shift, k)"""
    r = rng >> 16
    add = r * c_lo
    nl = low + add
    nr = rng - add if c_hi is None else r * (c_hi - c_lo)
    return nl >> 32, nl & M32, nr, _clz32(nr)


class CarryCoder:
    def __init__(self):
        self.low, self.rng, self.val, self.nbits = 0, M32, 0, 0
        self.carries, self.q = [], None

    def _carry(self, flush=False):
        t = _trailing_ones(self.val)
        assert t < self.nbits, "a carry out of the whole string: the interval left [0, 1)"
        self.carries.append(Carry(t, self.nbits % 32, self.nbits // 32, flush))
        self.val += 1

    def put(self, c_lo, c_hi):
        carry, nl, nr, k = cp_step(self.low, self.rng, c_lo, c_hi)
        assert nr > 0
        if carry:
            self._carry()
        if k:
            self.val = (self.val << k) | (nl >> (32 - k))
            self.nbits += k
        self.low, self.rng = (nl << k) & M32, nr << k

    def encode(self, rows, sym):
        for row, s in zip(rows, sym):
            self.put(*_slice_of(row, int(s)))
        return self

    def finish(self):
        self.q = (self.low + 0x3FFFFFFF) >> 30
        if self.q == 4:
            self._carry(flush=True)
        self.val, self.nbits = (self.val << 2) | (self.q & 3), self.nbits + 2
        return _bytes_of(self.val, self.nbits)


# ------------------------------------------------------------------------------------------------ carry-less
def rc_step(low, high, pending, c_lo, c_hi):
    """One symbol of rc_encode_core on (low, high, pending): (low, high, pending, n1, agreed bits, n2).  The n1 leading bits
    on which the new low and high agree leave first (E1 / E2; the first of them takes the pending run with it), then the
    interval is widened n2 times about the midpoint (E3) -- after an E3 step low < 2^31 <= high, so the order is fixed."""
    span = high - low + 1
    high = (low - 1 + ((span * (0x10000 if c_hi is None else c_hi)) >> 16)) & M32
    low = (low + ((span * c_lo) >> 16)) & M32
    n1 = bits = 0
    while high < MID or low >= MID:
        bits, n1 = (bits << 1) | (low >> 31), n1 + 1
        low, high = (low << 1) & M32, ((high << 1) | 1) & M32
    if n1:
        pending = 0
    n2 = 0
    while low >= 0x40000000 and high < 0xC0000000:
        low, high, n2 = (low << 1) & 0x7FFFFFFF, ((high << 1) | 0x80000001) & M32, n2 + 1
    return low, high, pending + n2, n1, bits, n2


class CarrylessCoder:
    def __init__(self):
        self.low, self.high, self.pending, self.val, self.nbits = 0, M32, 0, 0, 0
        self.resolutions = []

    def _emit(self, bit, rest, nrest, flush=False):
        """bit, `pending` copies of its complement, then the nrest further agreed bits"""
        self.resolutions.append(Resolution(self.pending, bit, nrest + 1, self.nbits % 32, flush))
        p = self.pending
        self.val = (((self.val << 1 | bit) << p) | (0 if bit else (1 << p) - 1)) << nrest | rest
        self.nbits += 1 + p + nrest

    def put(self, c_lo, c_hi):
        low, high, pending, n1, bits, _ = rc_step(self.low, self.high, self.pending, c_lo, c_hi)
        if n1:
            self._emit(bits >> (n1 - 1), bits & ((1 << (n1 - 1)) - 1), n1 - 1)
        self.low, self.high, self.pending = low, high, pending

    def encode(self, rows, sym):
        for row, s in zip(rows, sym):
            self.put(*_slice_of(row, int(s)))
        return self

    def finish(self):
        self.pending += 1
        self._emit(0 if self.low < 0x40000000 else 1, 0, 0, flush=True)
        return _bytes_of(self.val, self.nbits)


def model_encode(coder, rows, sym):
    """(bytes, the finished model) of one lane; coder = "carry" (version 4) or "carryless" """
    m = (CarryCoder if coder == "carry" else CarrylessCoder)().encode(rows, sym)
    return m.finish(), m


def longest_one_run(data):
    v = int.from_bytes(data, "big")
    return max((len(r) for r in bin(v)[2:].split("0")), default=0)


def longest_zero_run(data):
    return longest_one_run(bytes(b ^ 0xFF for b in data))


# ------------------------------------------------------------------------------------------------ rows
def _distinct(rs, lo, hi, k):
    """k distinct seeded integers of [lo, hi], ascending"""
    assert hi - lo + 1 >= k
    if hi - lo + 1 < 4 * k:
        return np.sort(rs.choice(hi - lo + 1, size=k, replace=False) + lo)
    while True:
        v = np.unique(rs.randint(lo, hi + 1, size=k))
        if len(v) == k:
            return v


def random_rows(rs, n, lp):
    """n seeded rows with lp - 2 distinct interior values, and uniform symbols"""
    rows = np.zeros((n, lp), np.uint16)
    for i in range(n):
        rows[i, 1:lp - 1] = _distinct(rs, 1, 65535, lp - 2)
    return rows, rs.randint(0, lp - 1, size=n).astype(np.uint8)


def _fits(lp, s, c_lo, c_hi):
    """can symbol s of a strictly ascending row take the slice [c_lo, c_hi)?"""
    if c_hi is None:
        return s == lp - 2 and s <= c_lo <= 65535
    if not (0 <= s < lp - 2 and c_lo < c_hi <= 65535 - (lp - 3 - s)):
        return False
    return c_lo == 0 if s == 0 else c_lo >= s


def _row_for(rs, lp, s, c_lo, c_hi):
    assert _fits(lp, s, c_lo, c_hi), (lp, s, c_lo, c_hi)
    row = np.zeros(lp, np.uint16)
    if s > 1:
        row[1:s] = _distinct(rs, 1, c_lo - 1, s - 1)
    row[s] = c_lo
    if c_hi is not None:
        row[s + 1] = c_hi
        k = lp - 3 - s
        if k:
            row[s + 2:lp - 1] = _distinct(rs, c_hi + 1, 65535, k)
    assert all(int(row[j]) < int(row[j + 1]) for j in range(lp - 2))
    return row


FLUSHES = ("flush", "flush_keep")
OFFS = sorted({0, 1, 2, 3, 5, 7} | {1 << j for j in range(2, 16)} | {3 << j for j in range(1, 14)})


class _Lane:
    """rows and symbols of one lane as they are chosen, with the model that has coded them"""
    def __init__(self, coder, lp, seed):
        self.coder, self.lp, self.rs = coder, lp, np.random.RandomState(seed)
        self.m = CarryCoder() if coder == "carry" else CarrylessCoder()
        self.rows, self.sym = [], []

    def add(self, s, c_lo, c_hi):
        self.rows.append(_row_for(self.rs, self.lp, s, c_lo, c_hi))
        self.sym.append(s)
        self.m.put(c_lo, c_hi)

    def _records(self):
        return self.m.carries if self.coder == "carry" else self.m.resolutions

    def mark(self):
        state = {k: v for k, v in vars(self.m).items() if k not in ("carries", "resolutions")}
        return len(self.sym), state, len(self._records())

    def rollback(self, mark):
        n, state, nrec = mark
        del self.rows[n:], self.sym[n:], self._records()[nrec:]
        vars(self.m).update(state)

    def add_row(self, row, s):
        self.rows.append(row)
        self.sym.append(int(s))
        self.m.put(*_slice_of(row, int(s)))

    def filler(self, n):
        rows, sym = random_rows(self.rs, n, self.lp)
        for row, s in zip(rows, sym):
            self.add_row(row, s)

    def slices(self, lo_edge, hi_edge, interior, lo_sign=-1, hi_sign=1):
        """candidate slices about the two edges: lo_edge + lo_sign * m as c_lo, hi_edge + hi_sign * m as c_hi; one-sided ones
        (c_lo = 0, or the last symbol) always, two-sided ones (an interior symbol) when asked for and Lp has any"""
        out = []
        for m in OFFS:
            out.append((0, hi_edge + hi_sign * m))
            out.append((lo_edge + lo_sign * m, None))
            if interior and self.lp > 3:
                out.append((lo_edge + lo_sign * m, hi_edge + hi_sign * m))
                out.append((lo_edge, hi_edge + hi_sign * m))
                out.append((lo_edge + lo_sign * m, hi_edge))
        return out

    def place(self, c_lo, c_hi):
        """a symbol whose slice this can be (a seeded choice among the interior ones), or None"""
        if c_lo < 0 or (c_hi is not None and not c_lo < c_hi <= 65535):
            return None
        fit = [s for s in ([self.lp - 2] if c_hi is None else [0] if c_lo == 0 else range(1, self.lp - 2)) if _fits(self.lp, s, c_lo, c_hi)]
        return fit[int(self.rs.randint(len(fit)))] if fit else None


# ------------------------------------------------------------------------------------------------ the carry coder's lanes
def _cp_after(m, c_lo, c_hi, B):
    """state after one straddling step: (trailing ones, low, range, B, k, range before the shift), or None when the slice
    leaves B.  No bit has left before the first shift (B = 2^31): the run starts behind the 0 that shift emits."""
    carry, nl, nr, k = cp_step(m.low, m.rng, c_lo, c_hi)
    if carry or nr <= 0 or not (nl < B < nl + nr):
        return None
    t = _trailing_ones(m.val) if B != MID else 0
    if k:
        bits = nl >> (32 - k)
        tb = _trailing_ones(bits)
        t = t + k if tb >= k else tb
        B = 1 << 32
    return t, (nl << k) & M32, nr << k, B, k, nr


def _cp_endings(lane, low, rng, B, ending, interior):
    """slices that end a straddle at (low, range): lift low to B or past it (carry), or stop at or below B (nocarry)"""
    r, D = rng >> 16, B - low
    out = []
    if ending == "carry":
        c = (D + r - 1) // r
        cands = ([(c, c + w) for w in (1, 2, 5, 300, 9000)] if interior and lane.lp > 3 else []) + [(c, None)]
        out = [(a, b) for a, b in cands if b is not None or r * a < rng]
    else:
        c = D // r
        cands = ([(c - w, c) for w in (1, 2, 5, 300, 9000)] if interior and lane.lp > 3 else []) + [(0, c)]
        out = [(a, b) for a, b in cands if 0 <= a < b]
    return [(a, b) for a, b in out if _fits_any(lane, a, b)]


def _fits_any(lane, c_lo, c_hi):
    lp = lane.lp
    if c_hi is None:
        return _fits(lp, lp - 2, c_lo, None)
    if c_lo == 0:
        return _fits(lp, 0, 0, c_hi)
    return lp > 3 and _fits(lp, min(c_lo, lp - 3), c_lo, c_hi)     # (the highest symbol c_lo admits leaves c_hi the most room)


def _retry(lane, fn, tries=40):
    """fn(attempt) from the same lane state until it succeeds (the lane's generator moves on, so attempts differ)"""
    mark = lane.mark()
    for attempt in range(tries):
        if fn(attempt):
            return True
        lane.rollback(mark)
    return False


def _cp_pad(lane, total):
    """symbols that emit exactly the bits missing to `total` and leave low < 2^31 (B = 2^31 lies in the interval then)"""
    return _retry(lane, lambda attempt: _cp_pad_once(lane, total))


def _cp_pad_once(lane, total):
    m, lp, rs = lane.m, lane.lp, lane.rs
    assert m.nbits <= total
    if m.nbits == total and m.low < MID:
        return True
    while m.nbits < total:
        rem = total - m.nbits
        for _ in range(400):
            b = int(min(rem, rs.randint(1, 9)))
            s = int(rs.randint(0, lp - 1))
            r = m.rng >> 16
            if s == lp - 2:
                c_lo, c_hi = int(rs.randint((m.rng - (1 << (32 - b))) // r + 1, (m.rng - (1 << (31 - b))) // r + 1)), None
            else:
                w = 1 << (16 - b)
                hi = 65535 - w - (lp - 3 - s)
                c_lo = 0 if s == 0 else int(rs.randint(s, hi + 1))
                c_hi = c_lo + w
            if not _fits(lp, s, c_lo, c_hi):
                continue
            carry, nl, nr, k = cp_step(m.low, m.rng, c_lo, c_hi)
            if k != b or nr <= 0 or (b == rem and ((nl << k) & M32) >= MID):
                continue
            lane.add(s, c_lo, c_hi)
            break
        else:
            return False
    return m.low < MID


def _cp_end_ok(lane, low, rng, B, ending, interior):
    if B == MID:
        return False
    if ending == "flush":
        return low > 0xC0000000                      # q = 4: the flush carries through the run
    if ending == "flush_keep":
        return 0 < low <= 0xC0000000                 # q < 4: the run stays, the flush's two bits follow it
    return bool(_cp_endings(lane, low, rng, B, ending, interior))


def _cp_straddle(lane, run, ending, interior, nsym=None):
    """narrow the interval about B until the string ends in exactly `run` ones, then the ending (or none: the flush).
    nsym = None: the longest step every time; else exactly nsym steps of about equal length (a lane that ends astride B
    has to end on its last symbol).  An attempt that runs into a state from which `run` cannot be met exactly is taken
    back, and the next attempts take a seeded random step now and then."""
    return _retry(lane, lambda attempt: _cp_straddle_once(lane, run, ending, interior, 0.0 if attempt == 0 else 0.3, nsym))


def _step_key(t, ta, run, left):
    """rank of a step from t to ta ones (or pending bits): the longest, or with `left` steps to go the one nearest an equal share"""
    return ta if left is None else -abs(ta - (t + -(-(run - t) // left)))


def _cp_straddle_once(lane, run, ending, interior, wander, nsym):
    m, B = lane.m, MID
    assert run >= 1 and m.low < B < m.low + m.rng
    for it in range(400):
        t = _trailing_ones(m.val) if B != MID else 0
        left = None if nsym is None else nsym - it
        if left == 0 or (left is None and t == run and _cp_end_ok(lane, m.low, m.rng, B, ending, interior)):
            break
        r, D = m.rng >> 16, B - m.low
        best, moves = None, []
        for c_lo, c_hi in lane.slices((D - 1) // r, D // r + 1, interior):
            if c_lo < 0 or (c_hi is not None and not c_lo < c_hi <= 65535) or not _fits_any(lane, c_lo, c_hi):
                continue
            a = _cp_after(m, c_lo, c_hi, B)
            if a is None or a[0] > run or (a[4] == 0 and not a[5] < m.rng):
                continue
            if left is not None and (run - a[0] < left - 1 or (left == 1 and a[0] != run)):
                continue                             # (at least a bit for each step still to come; the last one meets `run`)
            if a[0] == run and not _cp_end_ok(lane, a[1], a[2], a[3], ending, interior):
                continue
            key = (_step_key(t, a[0], run, left), a[4] > 0, c_hi is not None and c_lo != 0, -a[5])
            if a[4] > 0:
                moves.append((key, c_lo, c_hi, a))
            if best is None or key > best[0]:
                best = (key, c_lo, c_hi, a)
        if best is None:
            return False
        if moves and wander and lane.rs.rand() < wander:
            best = moves[int(lane.rs.randint(len(moves)))]
        _, c_lo, c_hi, a = best
        s = lane.place(c_lo, c_hi)
        if s is None:
            return False
        lane.add(s, c_lo, c_hi)
        B = a[3]
    else:
        return False
    if not (B != MID and _trailing_ones(m.val) == run and _cp_end_ok(lane, m.low, m.rng, B, ending, interior)):
        return False
    if ending not in FLUSHES:
        c_lo, c_hi = _cp_endings(lane, m.low, m.rng, B, ending, interior)[0]
        s = lane.place(c_lo, c_hi)
        if s is None:
            return False
        before = len(m.carries)
        lane.add(s, c_lo, c_hi)
        assert (len(m.carries) > before) == (ending == "carry")
    return True


# ------------------------------------------------------------------------------------------------ the carry-less coder's lanes
def _rc_edges(low, high):
    span = high - low + 1
    c_up = -((-((MID - low + 1) << 16)) // span)             # smallest c_hi with the new high >= 2^31
    c_dn = (((MID - low) << 16) - 1) // span                 # largest c_lo with the new low <= 2^31 - 1
    return c_dn, c_up


def _rc_endings(lane, low, high, pending, bit, long_n1, interior):
    """slices that resolve the pending run at (low, high) to `bit` with n1 == 1 (long_n1 False) or n1 > 1"""
    c_dn, c_up = _rc_edges(low, high)
    out = []
    for c_lo, c_hi in (lane.slices(c_dn, c_up - 1, interior, -1, -1) if bit == 0 else lane.slices(c_dn + 1, c_up, interior, 1, 1)):
        if c_lo < 0 or (c_hi is not None and not c_lo < c_hi <= 65535) or not _fits_any(lane, c_lo, c_hi):
            continue
        _, _, _, n1, bits, _ = rc_step(low, high, pending, c_lo, c_hi)
        if n1 and (bits >> (n1 - 1)) == bit and (n1 > 1) == long_n1:
            out.append((c_lo, c_hi))
    out.sort(key=lambda e: not (interior and e[0] != 0 and e[1] is not None))   # (stable: interior slices first when asked for)
    return out


def _rc_pad(lane, total):
    """seeded symbols until exactly `total` bits are written"""
    return _retry(lane, lambda attempt: _rc_pad_once(lane, total))


def _rc_pad_once(lane, total):
    m, lp, rs = lane.m, lane.lp, lane.rs
    assert m.nbits <= total
    while m.nbits < total:
        for _ in range(2000):
            rem = total - m.nbits
            b = int(rs.randint(1, min(rem, 8) + 1))
            s = int(rs.randint(0, lp - 1))
            w = 1 << (16 - b)
            if s == lp - 2:
                c_lo, c_hi = 65536 - w, None
            else:
                c_lo = 0 if s == 0 else int(rs.randint(s, 65535 - w - (lp - 3 - s) + 1))
                c_hi = c_lo + w
            if not _fits(lp, s, c_lo, c_hi):
                continue
            _, _, pend, n1, _, _ = rc_step(m.low, m.high, m.pending, c_lo, c_hi)
            written = m.nbits + (n1 + m.pending if n1 else 0)
            if written == total or written + pend + 1 <= total:
                lane.add(s, c_lo, c_hi)
                break
        else:
            return False
    return True


def _rc_straddle(lane, run, ending, long_n1, interior, nsym=None):
    """narrow [low, high] about the midpoint until `pending` == run, then resolve it (or leave it to the flush); nsym and
    the attempts as in _cp_straddle"""
    return _retry(lane, lambda attempt: _rc_straddle_once(lane, run, ending, long_n1, interior, 0.0 if attempt == 0 else 0.3, nsym))


def _rc_straddle_once(lane, run, ending, long_n1, interior, wander, nsym):
    m = lane.m
    bit = {"zero": 0, "one": 1}.get(ending)
    end_ok = lambda low, high, pend: ending == "flush" or bool(_rc_endings(lane, low, high, pend, bit, long_n1, interior))
    if m.pending > run:
        return False
    for it in range(400):
        left = None if nsym is None else nsym - it
        if left == 0 or (left is None and m.pending == run and end_ok(m.low, m.high, m.pending)):
            break
        c_dn, c_up = _rc_edges(m.low, m.high)
        best, moves = None, []
        for c_lo, c_hi in lane.slices(c_dn, c_up, interior):
            if c_lo < 0 or (c_hi is not None and not c_lo < c_hi <= 65535) or not _fits_any(lane, c_lo, c_hi):
                continue
            low, high, pend, n1, _, n2 = rc_step(m.low, m.high, m.pending, c_lo, c_hi)
            if n1 or pend > run or (n2 == 0 and not high - low < m.high - m.low):
                continue
            if left is not None and (run - pend < left - 1 or (left == 1 and pend != run)):
                continue
            if pend == run and not end_ok(low, high, pend):
                continue
            key = (_step_key(m.pending, pend, run, left), n2 > 0, c_hi is not None and c_lo != 0, low - high)
            if n2:
                moves.append((key, c_lo, c_hi))
            if best is None or key > best[0]:
                best = (key, c_lo, c_hi)
        if best is None:
            return False
        if moves and wander and lane.rs.rand() < wander:
            best = moves[int(lane.rs.randint(len(moves)))]
        _, c_lo, c_hi = best
        s = lane.place(c_lo, c_hi)
        if s is None:
            return False
        lane.add(s, c_lo, c_hi)
    else:
        return False
    if not (m.pending == run and end_ok(m.low, m.high, m.pending)):
        return False
    if ending != "flush":
        c_lo, c_hi = _rc_endings(lane, m.low, m.high, m.pending, bit, long_n1, interior)[0]
        s = lane.place(c_lo, c_hi)
        if s is None:
            return False
        lane.add(s, c_lo, c_hi)
        res = m.resolutions[-1]
        assert res.pending == run and res.bit == bit and (res.n1 > 1) == long_n1
    return True


# ------------------------------------------------------------------------------------------------ one lane
def _attempt(coder, lp, prefix_bits, run, ending, seed, interior, long_n1, lead, length=None):
    """filler, the bits up to the straddle's offset, the straddle; length: the straddle ends on the lane's last symbol"""
    lane = _Lane(coder, lp, seed)
    lane.filler(lead)
    m = lane.m
    # the straddle starts `prefix_bits` into the string (behind seeded filler: at that offset modulo 32)
    total = prefix_bits if not lead else m.nbits + (prefix_bits - m.nbits) % 32
    if coder == "carry":
        if not _cp_pad(lane, total) and not (lead and _cp_pad(lane, total + 32)):
            return None
    elif not _rc_pad(lane, total):
        return None
    start, nsym = m.nbits, None
    if length is not None:
        nsym = length - len(lane.sym)
        if nsym < 1:
            return None
    if not (_cp_straddle(lane, run, ending, interior, nsym) if coder == "carry" else _rc_straddle(lane, run, ending, long_n1, interior, nsym)):
        return None
    return lane, start


def make_lane(coder, lp, prefix_bits, run, ending, length, seed=0, interior=False, long_n1=False):
    """(rows (length, lp) uint16, symbols (length,) uint8, info) of one lane.

    coder        "carry" (version 4) or "carryless"
    prefix_bits  bits written before the straddle starts (carry: the offset of the 0 in front of the run of ones)
    run          carry: one bits in the string when the ending arrives; carryless: `pending` at its resolution
    ending       carry: "carry" | "nocarry" | "flush" (the lane ends astride B with low > 3 * 2^30: the flush's q = 4 carries
                 through the run) | "flush_keep" (the same with q < 4: the run stays);
                 carryless: "zero" | "one" (long_n1: with n1 > 1 agreed bits, else n1 == 1) | "flush"
    interior     Lp > 3: the straddling slices are interior symbols (both edges move in one step: the r * (c_hi - c_lo)
                 range branch); else symbol 0 and the last symbol (the range - add branch) take turns
    The construction stands at the lane's start and seeded filler follows it; with a flush ending the filler leads, and the
    straddle starts at prefix_bits modulo 32."""
    assert coder in ("carry", "carryless") and lp in (3, 5, 17)
    assert ending in (("carry", "nocarry", "flush", "flush_keep") if coder == "carry" else ("zero", "one", "flush"))
    got = None
    if ending not in FLUSHES:
        got = _attempt(coder, lp, prefix_bits, run, ending, seed, interior, long_n1, 0)
        if got is not None and len(got[0].sym) <= length:
            got[0].filler(length - len(got[0].sym))
        else:
            got = None
    else:
        # how many symbols the construction takes with the longest steps; then filler in front so that about half as many again are left
        first = _attempt(coder, lp, prefix_bits, run, ending, seed, interior, long_n1, 0)
        if first is not None:
            need = len(first[0].sym)
            for lead in range(length - need - max(2, need // 2), -1, -1):
                got = _attempt(coder, lp, prefix_bits, run, ending, seed, interior, long_n1, lead, length)
                if got is not None:
                    break
    if got is None:
        raise ValueError(f"no lane for {coder} lp={lp} prefix={prefix_bits} run={run} {ending} length={length} seed={seed}")
    lane, start = got[0], got[1]
    rows, sym = np.stack(lane.rows), np.array(lane.sym, np.uint8)
    assert rows.shape == (length, lp)
    return rows, sym, {"start": start}


# ------------------------------------------------------------------------------------------------ the generated set
# (prefix bits, run) of the version-4 lanes by lane length.  With the run's leading 0 at offset P, a carry through T ones
# arrives with W = P + 1 + T bits held: at position W % 32 of the device's accumulator, W // 32 words stored.
CARRY_RUNS = {
    64: [(0, 14),      # W = 15: ends inside the accumulator
         (1, 45),      # pos 15, 30 ones into the first stored word
         (31, 20),     # pos 20 = the run: the accumulator wraps, the 0 is the first word's last bit (a word boundary)
         (31, 52),     # pos 20: one whole word wraps, the 0 is the second word's last bit
         (31, 84),     # pos 20: two whole words wrap
         (0, 50),      # pos 19: the 0 is the first word's FIRST bit
         (32, 70),     # pos 7: the 0 is the second word's first bit
         (33, 100),    # pos 6: third word
         (0, 31),      # pos 0 (accumulator empty): first word
         (1, 62),      # pos 0: second word
         (0, 64),      # pos 1: second word
         (0, 62),      # pos 31: first word
         (0, 94)],     # pos 31: second word
    32: [(0, 14), (1, 45), (31, 52), (1, 62), (0, 64), (0, 31)],
    128: [(5, 260),    # pos 10: eighth word
          (31, 244),   # pos 20: seven whole words wrap, the 0 is the eighth word's last bit
          (0, 300)],   # pos 13: ninth word
}
CARRY_FLUSHES = {64: [(2, 70, "flush"), (7, 20, "flush"), (0, 40, "flush"), (2, 70, "flush_keep")],
                 32: [(3, 40, "flush")],
                 128: [(2, 240, "flush")]}
PENDING_RUNS = [31, 32, 33, 64, 100]
PENDING_PREFIX = [0, 1, 31, 32, 33]


def case_list(coder, length):
    """make_lane arguments (without lp / interior) of every generated lane of this length"""
    out = []
    if coder == "carry":
        for p, t in CARRY_RUNS[length]:
            out += [dict(prefix_bits=p, run=t, ending="carry"), dict(prefix_bits=p, run=t, ending="nocarry")]
        out += [dict(prefix_bits=p, run=t, ending=e) for p, t, e in CARRY_FLUSHES[length]]
    else:
        runs = PENDING_RUNS if length >= 64 else PENDING_RUNS[:4]
        for i, t in enumerate(runs):
            for j, (ending, long_n1) in enumerate((("zero", False), ("zero", True), ("one", False), ("one", True))):
                out.append(dict(prefix_bits=PENDING_PREFIX[(i + j) % 5], run=t, ending=ending, long_n1=long_n1))
        out += [dict(prefix_bits=PENDING_PREFIX[i % 5], run=t, ending="flush") for i, t in enumerate(runs[:4])]
    return out


_LANES = {}


def lanes(coder, lp, length):
    """[(case, rows, symbols)] of every generated lane of one coder, Lp and lane length (built once).  Lp > 3: cases take
    turns between interior straddling symbols and first / last ones (a carry / nocarry pair shares its choice)."""
    key = (coder, lp, length)
    if key not in _LANES:
        out = []
        for i, case in enumerate(case_list(coder, length)):
            interior = lp > 3 and ((i // 2) if coder == "carry" else i) % 2 == 0
            rows, sym, _ = make_lane(coder, lp, length=length, seed=1000 * lp + i, interior=interior, **case)
            out.append((dict(case, interior=interior), rows, sym))
        _LANES[key] = out
    return _LANES[key]


def plain_lane(lp, length, seed, zeros=False):
    """a lane of seeded filler; zeros: every symbol is 0, so `low` stays 0 (the version-4 flush's q = 0)"""
    rows, sym = random_rows(np.random.RandomState(seed), length, lp)
    return rows, (np.zeros(length, np.uint8) if zeros else sym)


# ------------------------------------------------------------------------------------------------ streams
def lane_log2(n, chunk_log2, version):
    """csrc/rc_format.hpp: rc_plan restated -- log2 of the symbols one coder state covers in a stream of n symbols"""
    assert chunk_log2 != 0
    clog = chunk_log2
    if version >= 2:
        per = 128 if version >= 3 else 256
        c = max((n + per - 1) // per - 1, 0).bit_length()           # ceil_log2(ceil(n / per))
        clog = min(max(c, min(chunk_log2, 7)), chunk_log2)
    return max(clog - 1 if version >= 3 else clog, 4)


def both_ways(lane_list, filler):
    """the lanes in an order that puts each of them once on an even slot (coded forwards) and once on an odd one (its bytes
    reversed); filler() gives the odd lane out.  Returns [(index into lane_list or None, rows, symbols)]."""
    seq = [(i,) + tuple(l) for i, l in enumerate(lane_list)]
    out = seq + ([(None,) + tuple(filler())] if len(seq) % 2 == 0 else []) + seq
    slots = {}
    for pos, e in enumerate(out):
        if e[0] is not None:
            slots.setdefault(e[0], set()).add(pos % 2)
    assert all(v == {0, 1} for v in slots.values()) and len(slots) == len(lane_list)
    return out
