"""Big-integer model of the reference's one-word fields (SmallFp<P> for Goldilocks, BabyBear, KoalaBear) and of the radix-2
domain over them.  Python integers only: constants by the Montgomery backend's rules, its three multiplication step sequences next
to the plain a * b * R^-1 mod p, the domain constructor and coset of poly/src/domain/radix2/mod.rs, a naive DFT, an iterative
radix-2 transform and Horner evaluation.  Elements are Montgomery residues ("as stored") unless a name says plain."""
import random

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


class Field:
    def __init__(self, name, sid, p, gen, word_bits):
        self.name, self.sid, self.p, self.gen_plain, self.word_bits = name, sid, p, gen, word_bits
        self.bytes = word_bits // 8
        # k_bits: the word's width; the backend hard-codes R = 2^32 for the two 31-bit fields (not 2^31)
        self.k_bits = word_bits
        self.R = 1 << self.k_bits
        self.r = self.R % p                       # one, as stored
        self.r2 = self.R * self.R % p
        self.rinv = pow(self.R, -1, p)
        self.nprime = (-pow(p, -1, self.R)) % self.R
        self.two_adicity = ((p - 1) & -(p - 1)).bit_length() - 1
        self.root_plain = pow(gen, (p - 1) >> self.two_adicity, p)
        self.root = self.root_plain * self.r % p
        self.gen = gen * self.r % p

    # ---- arithmetic on stored values ----
    def to_mont(self, x):
        return x % self.p * self.r % self.p

    def from_mont(self, a):
        return a * self.rinv % self.p

    def mul(self, a, b):
        return a * b * self.rinv % self.p

    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def pow(self, a, e):
        return self.to_mont(pow(self.from_mont(a), e, self.p))

    def inv(self, a):
        return self.pow(a, self.p - 2)

    # ---- the backend's step sequences (ff-macros/src/small_fp/montgomery_backend.rs), every intermediate wrapped as there ----
    def mul_steps(self, a, b):
        p = self.p
        if self.name == "GOLDILOCKS":
            t = a * b
            tl, th = t & M64, t >> 64
            k = tl + ((tl << 32) & M64)
            overflow, k = k >> 64, k & M64
            l = (k - (k >> 32) - overflow) & M64
            borrow = 1 if th < l else 0
            r = (th - l) & M64
            r = (r - ((0 - borrow) & M32)) & M64
            return r - p if r >= p else r
        sh = 27 if self.name == "BABYBEAR" else 24
        t = a * b
        t32 = t & M32
        k = (((t32 << 31) & M32) - ((t32 << sh) & M32) - t32) & M32
        kp = (((k << 31) & M64) - ((k << sh) & M64) + k) & M64
        r = ((t + kp) & M64) >> self.k_bits
        return r - p if r >= p else r

    def mul_generic_steps(self, a, b):
        """the textbook sequence with t * N' as a product: what a device multiply may use instead of the shift forms"""
        t = a * b
        m = (t & (self.R - 1)) * self.nprime & (self.R - 1)
        r = (t + m * self.p) >> self.k_bits
        return r - self.p if r >= self.p else r

    def edge_values(self):
        p = self.p
        vals = [0, 1, 2, p - 1, p - 2, M32, 1 << 32, (1 << 32) + 1, self.r]
        return sorted({v for v in vals if v < p})

    def random_elements(self, rng, n):
        return [rng.randrange(self.p) for _ in range(n)]

    # ---- domains (radix2/mod.rs:55-92) ----
    def domain_new(self, num_coeffs):
        size = 1
        while size < num_coeffs:
            size <<= 1
        log = size.bit_length() - 1
        if log > self.two_adicity:
            return None
        w = self.root
        for _ in range(log, self.two_adicity):
            w = self.mul(w, w)
        sfe = self.to_mont(size)
        return dict(size=size, log_size_of_group=log, size_as_field_element=sfe, size_inv=self.inv(sfe), group_gen=w,
                    group_gen_inv=self.inv(w), offset=self.r, offset_inv=self.r, offset_pow_size=self.r)

    def get_coset(self, dom, offset):
        if offset == 0:
            return None
        d = dict(dom)
        d.update(offset=offset, offset_inv=self.inv(offset), offset_pow_size=self.pow(offset, dom["size"]))
        return d

    # ---- transforms: coefficient i scaled by offset^i, then evaluated at the powers of group_gen ----
    def _plain(self, xs):
        return [self.from_mont(x) for x in xs]

    def _dft(self, v, w):
        n, p = len(v), self.p
        pw = [1] * n
        for t in range(1, n):
            pw[t] = pw[t - 1] * w % p
        return [sum(c * pw[i * j % n] for i, c in enumerate(v)) % p for j in range(n)]

    def dft_naive(self, dom, xs, inverse=False):
        """O(n^2), from the definition; xs as stored, zero-extended to the domain"""
        p, n = self.p, dom["size"]
        v = self._plain(xs) + [0] * (n - len(xs))
        if not inverse:
            h, w = self.from_mont(dom["offset"]), self.from_mont(dom["group_gen"])
            v = [c * pow(h, i, p) % p for i, c in enumerate(v)]
            out = self._dft(v, w)
        else:
            hi, wi, ni = self.from_mont(dom["offset_inv"]), self.from_mont(dom["group_gen_inv"]), self.from_mont(dom["size_inv"])
            out = self._dft(v, wi)
            out = [c * ni % p * pow(hi, j, p) % p for j, c in enumerate(out)]
        return [self.to_mont(c) for c in out]

    def fft_fast(self, dom, xs, inverse=False):
        """iterative radix-2 (decimation in time on plain integers), for sizes the naive sum is too slow for"""
        p, n, log = self.p, dom["size"], dom["log_size_of_group"]
        v = self._plain(xs) + [0] * (n - len(xs))
        if not inverse:
            h = self.from_mont(dom["offset"])
            if h != 1:
                acc = 1
                for i in range(n):
                    v[i] = v[i] * acc % p
                    acc = acc * h % p
            w = self.from_mont(dom["group_gen"])
        else:
            w = self.from_mont(dom["group_gen_inv"])
        a = [0] * n
        for i in range(n):
            a[int(format(i, "0%db" % log)[::-1], 2) if log else 0] = v[i]
        half = 1
        while half < n:
            wm = pow(w, n // (2 * half), p)
            tw = [1] * half
            for j in range(1, half):
                tw[j] = tw[j - 1] * wm % p
            for start in range(0, n, 2 * half):
                for j in range(half):
                    u, t = a[start + j], a[start + j + half] * tw[j] % p
                    a[start + j] = (u + t) % p
                    a[start + j + half] = (u - t) % p
            half *= 2
        if inverse:
            ni, hi = self.from_mont(dom["size_inv"]), self.from_mont(dom["offset_inv"])
            acc = ni
            for j in range(n):
                a[j] = a[j] * acc % p
                acc = acc * hi % p
        return [self.to_mont(c) for c in a]

    def transform(self, dom, xs, inverse=False):
        return self.dft_naive(dom, xs, inverse) if dom["size"] <= 512 else self.fft_fast(dom, xs, inverse)

    def horner(self, coeffs, x):
        """the polynomial with these stored coefficients at the stored point x, as stored"""
        p = self.p
        xp, acc = self.from_mont(x), 0
        for c in reversed(coeffs):
            acc = (acc * xp + self.from_mont(c)) % p
        return self.to_mont(acc)

    def domain_element(self, dom, j):
        return self.mul(dom["offset"], self.pow(dom["group_gen"], j))


GOLDILOCKS = Field("GOLDILOCKS", 0, 2**64 - 2**32 + 1, 7, 64)
BABYBEAR = Field("BABYBEAR", 1, 2**31 - 2**27 + 1, 31, 32)
KOALABEAR = Field("KOALABEAR", 2, 2**31 - 2**24 + 1, 3, 32)
FIELDS = {f.name: f for f in (GOLDILOCKS, BABYBEAR, KOALABEAR)}

DOMAIN_KEYS = ("size", "log_size_of_group", "size_as_field_element", "size_inv", "group_gen", "group_gen_inv", "offset", "offset_inv",
               "offset_pow_size")


def rng(seed):
    return random.Random(seed)
