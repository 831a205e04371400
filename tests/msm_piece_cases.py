"""Input families of the streamed-piece tests (test_msm_bucket_host.py without a GPU, test_gpu_msm_pieces.py on the device): each
puts one branch of the `accum` paths of csrc/msm.cuh on a piece boundary.  A Case names its regime -- which cells are heavy in
which piece, which pieces are empty -- and both test files assert it from the model (the GPU file from the dumped counters too).

Bases are [k] G with k = A + i B; edited entries are duplicates (the same k), negatives (r - k), sums (k_a + k_b) and the
identity (None).  A small scalar d <= 2^(c-1) - 1 has the digit d in window 0 and none elsewhere: it lands in bucket d - 1 of
window 0; r - d lands there negated."""
import random

import msm_bucket_ref as BR
import msm_sort_ref as R

A0, B0 = 0xA11CE + (1 << 64) + (2 << 128), 0xB0B + (3 << 64)
G1 = ("BN254_G1", "BLS12_381_G1", "BLS12_377_G1")
G2 = ("BLS12_377_G2", "BLS12_381_G2")


class Case:
    def __init__(self, name, inp, c, heavy=0, lazy=1, heavy_cells=None, empty=(), all_identity=(), runs=None):
        self.name, self.inp, self.c, self.heavy, self.lazy = name, inp, c, heavy, lazy
        self.heavy_cells = heavy_cells   # per piece: the cells (window 0 buckets) whose runs are heavy; None: not pinned
        self.empty = tuple(empty)        # pieces without a single digit: the bucket array must not change by a byte
        self.all_identity = tuple(all_identity)   # pieces after which every bucket is the identity
        self.runs = runs                 # per piece (items, runs, threshold) where the case pins them

    def knobs(self):
        return dict(c=self.c, heavy=self.heavy, lazy=self.lazy)

    def model(self, header=None):
        h = header or BR.plan_header(self.inp.curve, self.c, self.inp.sizes)
        return BR.BucketModel(self.inp, h, self.heavy)

    def __repr__(self):
        return self.name


def logs(n, start=0):
    return [A0 + (start + i) * B0 for i in range(n)]


def uniform(curve, n, seed):
    r = BR.CurveRef(curve).r
    rng = random.Random(seed)
    return [rng.randrange(1, r) for _ in range(n)]


def to_mont(curve, scalars):
    import pyref
    r = BR.CurveRef(curve).r
    return [s * pyref.R_of(r) % r for s in scalars]


class Builder:
    """pairs appended piece by piece"""

    def __init__(self, curve):
        self.curve, self.r = curve, BR.CurveRef(curve).r
        self.logs, self.scalars, self.sizes, self.fresh = [], [], [], 0
        self.open = 0

    def new(self, count=1):
        """logs of `count` bases not used before"""
        out = logs(count, self.fresh)
        self.fresh += count
        return out

    def add(self, log, scalar):
        self.logs.append(log)
        self.scalars.append(scalar % (1 << 256))
        self.open += 1

    def run(self, d, count, neg=False, logs_=None):
        """`count` entries for bucket d - 1 of window 0 (negated: scalar r - d); returns their logs"""
        ls = self.new(count) if logs_ is None else logs_
        for k in ls:
            self.add(k, self.r - d if neg else d)
        return ls

    def background(self, count, seed, logs_=None):
        """full-width scalars with no digit in window 0 (magnitude a multiple of 2^8 >= 2^c), every other one folded (r - s)"""
        rng = random.Random(seed)
        for i, k in enumerate(self.new(count) if logs_ is None else logs_):
            s = rng.randrange(1, self.r >> 9) << 8
            self.add(k, self.r - s if i % 2 else s)

    def cut(self):
        assert self.open
        self.sizes.append(self.open)
        self.open = 0

    def input(self, mont=0):
        assert not self.open
        sc = to_mont(self.curve, self.scalars) if mont else self.scalars
        return BR.Input(self.curve, self.logs, sc, self.sizes, mont)


# ---- baseline ----------------------------------------------------------------------------------------------------------------
def baseline(curve, mont, lazy=1):
    n = 2502
    sc = uniform(curve, n, 7 + mont)
    inp = BR.Input(curve, logs(n), to_mont(curve, sc) if mont else sc, [1000, 1, 1501], mont)
    return Case("baseline-%s-mont%d%s" % (curve, mont, "" if lazy else "-saturated"), inp, 8, lazy=lazy, heavy_cells=[[], [], []])


def edge_values(curve="BLS12_381_G1", c=8):
    """the sort-stage test's edge scalars, each in a later piece than a uniform first one"""
    cr = BR.CurveRef(curve)
    r, bits = cr.r, cr.bits
    W, narrow = R.layout(c, bits)
    chain, off = 0, 0
    for cw in R.window_widths(c, W, narrow):   # every window exactly half: the carry chain
        chain |= (1 << (cw - 1)) << off
        off += cw
    chain %= r
    vals = [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2, chain, chain - 1, chain + 1, r - chain, 2, r - 2, r, r + 1, (1 << bits) - 1]
    sc = uniform(curve, 300, 3)
    sc[100:100 + len(vals)] = vals                 # piece 1
    sc[200 + 7:200 + 7 + len(vals)] = vals[::-1]   # piece 2, other bases
    return Case("edge-values", BR.Input(curve, logs(300), sc, [100, 100, 100]), c, heavy_cells=[[], [], []])


# ---- empty pieces ------------------------------------------------------------------------------------------------------------
def empty_pieces(curve, first_is_r, lazy=1):
    """pieces of scalars that are all 0 or all r first, in the middle and last"""
    b = Builder(curve)
    r = b.r
    fill = [r, 0, r] if first_is_r else [0, r, 0]
    for k in range(5):
        if k % 2 == 0:
            for log in b.new(40):
                b.add(log, fill[k // 2])
        else:
            b.background(150, 20 + k)
        b.cut()
    return Case("empty-%s-%s%s" % (curve, "r0r" if first_is_r else "0r0", "" if lazy else "-saturated"), b.input(), 6, lazy=lazy,
                empty=(0, 2, 4), all_identity=(0,))


# ---- threshold and chunk edges -------------------------------------------------------------------------------------------------
def threshold_edges(heavy=0, curve="BLS12_381_G1"):
    """runs of 64, 65, 1024 and 1025 entries in buckets 0 .. 3 of window 0, every third entry negated"""
    b = Builder(curve)
    for d, count in ((1, 64), (2, 65), (3, 1024), (4, 1025)):
        for i, log in enumerate(b.new(count)):
            b.add(log, b.r - d if i % 3 == 2 else d)
    b.cut()
    if heavy == 0:
        return Case("threshold-edges", b.input(), 5, heavy_cells=[[1, 2, 3]], runs=[(4, 3, 64)])
    return Case("threshold-edges-heavy%d" % heavy, b.input(), 5, heavy=heavy, heavy_cells=[[3]], runs=[(2, 1, heavy)])


# ---- heavy and light alternate on one cell -----------------------------------------------------------------------------------
def alternating(curve, pieces=3, light=9, heavy=70, background=40, equal=False):
    """bucket 0: light, heavy, light, ..; bucket 1: heavy, light, heavy, ..; bucket 2: heavy in every piece (equal: pieces of one size)"""
    b = Builder(curve)
    cells = []
    for k in range(pieces):
        b.run(1, heavy if k % 2 else light, neg=k == 2)
        b.run(2, light if k % 2 else heavy)
        b.run(3, heavy if equal else heavy + k)
        if background:
            b.background(background, 30 + k)
        b.cut()
        cells.append([0, 2] if k % 2 else [1, 2])
    return Case("alternating-%s-%d" % (curve, pieces), b.input(), 5, heavy_cells=cells)


# ---- doubling and cancelling on the boundary, lane path ------------------------------------------------------------------------
def lane_boundary(curve, lazy=1):
    """piece 0 leaves P (ZZ = 1) or S = P_a + P_b (ZZ != 1) in a bucket; piece 1's entries for it are that very point, or its
    negative; piece 2 adds one more entry to every one of these buckets (onto 2 P, 2 S, and onto the stored identity)"""
    b = Builder(curve)
    r = b.r
    (p1,), (p2,), (p5,), (p6,) = b.run(1, 1), b.run(2, 1), b.run(5, 1), b.run(6, 1)   # one base each: stored with ZZ = 1
    s3, s4, s7 = b.run(3, 2), b.run(4, 2), b.run(7, 2)                                 # two bases each: S, ZZ != 1
    b.background(30, 41)
    b.cut()
    b.run(1, 1, logs_=[p1])                        # P + P: the equal-point branch right on the loaded value
    b.run(2, 1, neg=True, logs_=[p2])              # P - P: the identity
    b.run(3, 1, logs_=[sum(s3) % r])               # S + S through the base whose affine point is S
    b.run(4, 1, neg=True, logs_=[sum(s4) % r])     # S - S
    b.run(5, 1, logs_=[p5])                        # P + P, then a further entry in the same piece
    b.run(5, 1)
    b.run(6, 1, neg=True, logs_=[p6])              # P - P, then a further entry added onto the identity in the same piece
    b.run(6, 1)
    b.run(7, 1, neg=True, logs_=[sum(s7) % r])     # S - S, then a further entry
    b.run(7, 1)
    b.background(30, 42)
    b.cut()
    for d in range(1, 8):
        b.run(d, 1)
    b.cut()
    return Case("lane-boundary-%s%s" % (curve, "" if lazy else "-saturated"), b.input(), 5, lazy=lazy, heavy_cells=[[], [], []])


# ---- doubling and cancelling on the boundary, heavy path -----------------------------------------------------------------------
def heavy_boundary(curve):
    """piece 1's heavy runs repeat piece 0's pairs (acc == prev), their negated scalars (-> the identity), or add onto a stored
    identity -- one that no entry ever reached, and one that piece 0 cancelled to"""
    b = Builder(curve)
    same = b.run(1, 70)                            # heavy in piece 0
    opp = b.run(2, 70)
    lane_same = b.run(5, 9)                        # light in piece 0 (a lane wrote the cell), heavy in piece 1
    (q,) = b.run(4, 1)
    b.run(4, 1, neg=True, logs_=[q])               # bucket 3 cancels to the identity inside piece 0
    b.background(30, 51)
    b.cut()
    b.run(1, 70, logs_=same)                       # the run sums to exactly what is stored
    b.run(2, 70, neg=True, logs_=opp)              # ... to its negative
    b.run(3, 70)                                   # onto the identity nothing ever touched
    b.run(4, 70)                                   # onto the identity piece 0 left
    for _ in range(8):                             # 72 entries that sum to 8 x the stored point: not equal, heavy after light
        b.run(5, 9, logs_=lane_same)
    b.background(30, 52)
    b.cut()
    return Case("heavy-boundary-%s" % curve, b.input(), 5, heavy_cells=[[0, 1], [0, 1, 2, 3, 4]])


# ---- the whole array cancels -------------------------------------------------------------------------------------------------
def cancelling(curve, two_valued, n=400, pieces=2, c=6):
    """piece 2 j + 1 is piece 2 j with every scalar s replaced by r - s: every bucket is the identity behind each odd piece"""
    cr = BR.CurveRef(curve)
    rng = random.Random(61)
    if two_valued:
        a, bb = rng.randrange(1, cr.r), rng.randrange(1, cr.r)
        sc = [a if rng.random() < 0.8 else bb for _ in range(n)]
    else:
        sc = uniform(curve, n, 62)
    ls, scalars, all_logs = logs(n), [], []
    for k in range(pieces):
        scalars += sc if k % 2 == 0 else [cr.r - s for s in sc]
        all_logs += ls
    odd = tuple(range(1, pieces, 2))
    return Case("cancelling-%s-%s-%d" % (curve, "two" if two_valued else "uniform", pieces),
                BR.Input(curve, all_logs, scalars, [n] * pieces), c, all_identity=odd)


def two_valued(curve, n, pieces, c=6):
    """88 % one scalar, 10 % another, the rest uniform: a heavy run in every window of every piece"""
    cr = BR.CurveRef(curve)
    rng = random.Random(71)
    a, bb = rng.randrange(1, cr.r), rng.randrange(1, cr.r)
    sc = uniform(curve, n, 72)
    for i in range(n):
        u = rng.random()
        if u < 0.88:
            sc[i] = a
        elif u < 0.98:
            sc[i] = bb
    step = -(-n // pieces)
    sizes = [min(step, n - o) for o in range(0, n, step)]
    return Case("two-valued-%s-%d" % (curve, pieces), BR.Input(curve, logs(n), sc, sizes), c)


# ---- identity bases ----------------------------------------------------------------------------------------------------------
def identity_bases(curve="BLS12_381_G1"):
    """every third base is the identity; a heavy run made of identities only; a piece made of identities only"""
    b = Builder(curve)
    b.background(300, 81, [None if i % 3 == 0 else log for i, log in enumerate(b.new(300))])
    b.run(1, 70, logs_=[None] * 70)                # bucket 0 of window 0: a heavy run of 70 identities and nothing else
    b.run(2, 70)
    b.cut()
    b.background(100, 82, [None] * 100)
    b.cut()
    b.background(300, 83, [None if i % 3 == 1 else log for i, log in enumerate(b.new(300))])
    b.run(1, 70, logs_=[None] * 70)
    b.cut()
    return Case("identity-bases", b.input(), 6)


# ---- range flag --------------------------------------------------------------------------------------------------------------
def out_of_range(curve, piece, pieces=3, n_piece=120):
    cr = BR.CurveRef(curve)
    n = pieces * n_piece
    sc = uniform(curve, n, 91)
    sc[piece * n_piece + 17] = 1 << cr.bits
    return Case("out-of-range-%d" % piece, BR.Input(curve, logs(n), sc, [n_piece] * pieces), 6)


def bucket_cases():
    """every case of the bucket-level GPU tests (the host file folds each against the oracle and asserts its regime)"""
    cases = [baseline(cv, mont) for cv in R.CURVES for mont in (0, 1)]
    cases += [edge_values()]
    cases += [empty_pieces("BLS12_381_G1", False), empty_pieces("BLS12_381_G1", True)]
    cases += [threshold_edges(0), threshold_edges(1024)]
    cases += [alternating("BLS12_381_G1"), lane_boundary("BLS12_381_G1"), heavy_boundary("BLS12_381_G1")]
    cases += [cancelling("BLS12_381_G1", False), cancelling("BLS12_381_G1", True), identity_bases()]
    for cv in G2:
        cases += [alternating(cv, background=10), lane_boundary(cv), heavy_boundary(cv)]
    for cv in ("BLS12_381_G1", "BN254_G1"):
        cases += [baseline(cv, 0, lazy=0), empty_pieces(cv, False, lazy=0), empty_pieces(cv, True, lazy=0), lane_boundary(cv, lazy=0)]
    return cases


def self_cancelling_pieces(curve, pieces=17, m=40, c=6):
    """`pieces` pieces of m pairs; pieces 3 and 4 each hold m / 2 pairs and the same bases with the negated scalars: cut into
    independent MSMs, both return the identity"""
    b = Builder(curve)
    for k in range(pieces):
        if k in (3, 4):
            ls, sc = b.new(m // 2), uniform(curve, m // 2, 100 + k)
            for log, s in zip(ls, sc):
                b.add(log, s)
            for log, s in zip(ls, sc):
                b.add(log, b.r - s)
        else:
            for log, s in zip(b.new(m), uniform(curve, m, 100 + k)):
                b.add(log, s)
        b.cut()
    return Case("self-cancelling-%s-%d" % (curve, pieces), b.input(), c)
