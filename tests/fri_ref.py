"""Big-integer model of the extension fields over the one-word fields and of FRI over them (include/ark_hip.h, DESIGN.md section
30).  Python integers only, no code of the library; its own Montgomery constants, as smallfp_ref.py has.

    Goldilocks             Fp2 = Fp[u] / (u^2 - 7)
    BabyBear / KoalaBear   Fp4 = Fp2[v] / (v^2 - u), Fp2 = Fp[u] / (u^2 - W), W = 11 / 3

An element is a tuple of d residues in the order CanonicalSerialize writes them (c0, c1 / c0.c0, c0.c1, c1.c0, c1.c1).  The
arithmetic below works on PLAIN residues; `stored` / `plain` move whole elements, vectors ([d][n] lists) and rows in and out of
Montgomery form, which is what memory and every hash hold."""
import hashlib
import random

import merkle_ref as MR


class ExtField:
    def __init__(self, name, sid, p, gen, word_bits, w, d):
        self.name, self.sid, self.p, self.gen, self.w, self.d = name, sid, p, gen, w, d
        self.bytes = word_bits // 8
        self.R = (1 << word_bits) % p            # R = 2^64, and 2^32 for both 31-bit fields
        self.rinv = pow(self.R, -1, p)
        self.two_adicity = ((p - 1) & -(p - 1)).bit_length() - 1
        self.root = pow(gen, (p - 1) >> self.two_adicity, p)
        # component k is the coefficient of X^expo[k] in Fp[X] / (X^d - W)
        self.expo = (0, 1) if d == 2 else (0, 2, 1, 3)

    # ---- Montgomery form ----
    def st(self, x):
        return x * self.R % self.p

    def pl(self, s):
        return s * self.rinv % self.p

    def stored(self, e):
        return tuple(self.st(x) for x in e)

    def plain(self, e):
        return tuple(self.pl(x) for x in e)

    def vec_plain(self, v):      # [d][n] stored -> list of n plain elements
        return [tuple(self.pl(v[k][i]) for k in range(self.d)) for i in range(len(v[0]))]

    def vec_stored(self, elems):   # list of plain elements -> [d][n] stored
        return [[self.st(e[k]) for e in elems] for k in range(self.d)]

    # ---- tower arithmetic, plain ----
    def zero(self):
        return (0,) * self.d

    def one(self):
        return (1,) + (0,) * (self.d - 1)

    def base(self, x):
        return (x % self.p,) + (0,) * (self.d - 1)

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % self.p for x in a)

    def scale(self, a, s):
        return tuple(x * s % self.p for x in a)

    def _mul2(self, a, b):
        p = self.p
        return ((a[0] * b[0] + self.w * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def _inv2(self, a):
        p = self.p
        n = (a[0] * a[0] - self.w * a[1] * a[1]) % p
        ni = pow(n, p - 2, p)                    # 0 -> 0
        return (a[0] * ni % p, -a[1] * ni % p)

    def mul(self, a, b):
        if self.d == 2:
            return self._mul2(a, b)
        c0, c1, d0, d1 = a[:2], a[2:], b[:2], b[2:]
        v0, v1 = self._mul2(c0, d0), self._mul2(c1, d1)
        v1u = (self.w * v1[1] % self.p, v1[0])               # times u
        x = self._mul2(c0, d1)
        y = self._mul2(c1, d0)
        return ((v0[0] + v1u[0]) % self.p, (v0[1] + v1u[1]) % self.p, (x[0] + y[0]) % self.p, (x[1] + y[1]) % self.p)

    def inv(self, a):
        """by the norm down the tower; zero maps to zero"""
        if self.d == 2:
            return self._inv2(a)
        c0, c1 = a[:2], a[2:]
        s0, s1 = self._mul2(c0, c0), self._mul2(c1, c1)
        n = ((s0[0] - self.w * s1[1]) % self.p, (s0[1] - s1[0]) % self.p)
        ni = self._inv2(n)
        r0, r1 = self._mul2(c0, ni), self._mul2(c1, ni)
        return (r0[0], r0[1], -r1[0] % self.p, -r1[1] % self.p)

    def pow(self, a, e):
        r = self.one()
        while e:
            if e & 1:
                r = self.mul(r, a)
            a = self.mul(a, a)
            e >>= 1
        return r

    # ---- the same product as polynomials modulo X^d - W ----
    def to_poly(self, a):
        x = [0] * self.d
        for k in range(self.d):
            x[self.expo[k]] = a[k]
        return x

    def from_poly(self, x):
        return tuple(x[self.expo[k]] for k in range(self.d))

    def mul_poly(self, a, b):
        d, p = self.d, self.p
        x, y = self.to_poly(a), self.to_poly(b)
        prod = [0] * (2 * d - 1)
        for i in range(d):
            for j in range(d):
                prod[i + j] += x[i] * y[j]
        for t in range(2 * d - 2, d - 1, -1):                # X^t = W X^(t - d)
            prod[t - d] += self.w * prod[t]
        return self.from_poly([c % p for c in prod[:d]])

    def w_is_irreducible(self):
        """W a non-square (Euler) and, for d = 4, p = 1 mod 4: then X^4 - W has no root and no quadratic factor"""
        p = self.p
        return pow(self.w, (p - 1) // 2, p) == p - 1 and (self.d == 2 or p % 4 == 1)

    def random_element(self, rng):
        return tuple(rng.randrange(self.p) for _ in range(self.d))

    # ---- domains, plain: D = { h w^i }, w of order 2^k ----
    def omega(self, k):
        return pow(self.root, 1 << (self.two_adicity - k), self.p)

    def fold2(self, f, k, h, beta):
        """one 2-fold by the evaluation formula: n = 2^k plain elements over h <w> -> n / 2 over h^2 <w^2>"""
        p, n = self.p, 1 << k
        w, half = self.omega(k), n // 2
        inv2 = pow(2, p - 2, p)
        out = []
        x = h
        for i in range(half):
            s = self.scale(self.add(f[i], f[i + half]), inv2)
            dlt = self.scale(self.sub(f[i], f[i + half]), pow(2 * x, p - 2, p))
            out.append(self.add(s, self.mul(beta, dlt)))
            x = x * w % p
        return out

    def fold_eval(self, f, k, h, a, beta):
        """arity 2^a as a successive 2-folds with beta, beta^2, beta^4"""
        for _ in range(a):
            f = self.fold2(f, k, h, beta)
            k, h, beta = k - 1, h * h % self.p, self.mul(beta, beta)
        return f

    def interpolate(self, f, k, h):
        """coefficients of the polynomial of degree < n with these values over h <w>, naively"""
        p, n = self.p, 1 << k
        wi, ni, hi = pow(self.omega(k), p - 2, p), pow(n, p - 2, p), pow(h, p - 2, p)
        pw = [pow(wi, t, p) for t in range(n)]
        out = []
        for j in range(n):
            acc = self.zero()
            for i in range(n):
                acc = self.add(acc, self.scale(f[i], pw[i * j % n]))
            out.append(self.scale(acc, ni * pow(hi, j, p) % p))
        return out

    def evaluate(self, coeffs, k, h):
        p, n = self.p, 1 << k
        w = self.omega(k)
        out = []
        for i in range(n):
            x = h * pow(w, i, p) % p
            acc = self.zero()
            for c in reversed(coeffs):
                acc = self.add(self.scale(acc, x), c)
            out.append(acc)
        return out

    def fold_coeff(self, f, k, h, a, beta):
        """the definition: f(X) = sum_r X^r f_r(X^(2^a)), g = sum_r beta^r f_r over h^(2^a) <w^(2^a)>"""
        c = self.interpolate(f, k, h)
        m, r = 1 << (k - a), 1 << a
        g = []
        for t in range(m):
            acc, bp = self.zero(), self.one()
            for j in range(r):
                acc = self.add(acc, self.mul(bp, c[t * r + j]))
                bp = self.mul(bp, beta)
            g.append(acc)
        return self.evaluate(g, k - a, pow(h, r, self.p))

    def combine(self, cols, alpha, first_power=0, acc=None):
        """out[i] = acc[i] + alpha^first_power sum_j alpha^j cols[j][i]; cols plain base-field lists"""
        rows = len(cols[0])
        out = []
        pws = [self.pow(alpha, first_power)]
        for _ in range(len(cols) - 1):
            pws.append(self.mul(pws[-1], alpha))
        for i in range(rows):
            v = acc[i] if acc is not None else self.zero()
            for j, col in enumerate(cols):
                v = self.add(v, self.scale(pws[j], col[i]))
            out.append(v)
        return out

    # ---- the commit phase on stored data ----
    def row_view(self, layer, a):
        """[d][n] stored -> the d 2^a columns of n / 2^a rows: column k 2^a + j holds component k of f[. + j n / 2^a]"""
        n = len(layer[0])
        m = n >> a
        return [layer[k][j * m:(j + 1) * m] for k in range(self.d) for j in range(1 << a)]

    def layer_arities(self, k, a, num_folds):
        out = []
        for _ in range(num_folds):
            al = min(a, k)
            assert al >= 1
            out.append(al)
            k -= al
        return out

    def commit_phase(self, layer0, k, h, a, num_folds, challenge_fn):
        """layer0 [d][n] stored, h plain.  Returns dict(layers=[...stored], trees=[lists of digests], roots, betas (stored), final
        ([d][size] stored coefficients), arities, offsets (plain h per layer))"""
        layers, trees, roots, betas, offs = [layer0], [], [], [], [h]
        ar = self.layer_arities(k, a, num_folds)
        for al in ar:
            t = MR.tree(self.name, self.row_view(layers[-1], al))
            trees.append(t)
            roots.append(t[0])
            beta_s = tuple(challenge_fn(t[0]))
            betas.append(beta_s)
            g = self.fold_eval(self.vec_plain(layers[-1]), k, h, al, self.plain(beta_s))
            layers.append(self.vec_stored(g))
            k, h = k - al, pow(h, 1 << al, self.p)
            offs.append(h)
        final = self.vec_stored(self.interpolate_fast(self.vec_plain(layers[-1]), k, h))
        return dict(layers=layers, trees=trees, roots=roots, betas=betas, final=final, arities=ar, offsets=offs, last_log=k)

    def interpolate_fast(self, f, k, h):
        """as interpolate, by an iterative radix-2 transform (sizes the naive sum is too slow for)"""
        p, n = self.p, 1 << k
        if n <= 64:
            return self.interpolate(f, k, h)
        wi = pow(self.omega(k), p - 2, p)
        a = [None] * n
        for i in range(n):
            a[int(format(i, "0%db" % k)[::-1], 2)] = f[i]
        half = 1
        while half < n:
            wm = pow(wi, n // (2 * half), p)
            tw = [1] * half
            for j in range(1, half):
                tw[j] = tw[j - 1] * wm % p
            for start in range(0, n, 2 * half):
                for j in range(half):
                    u, t = a[start + j], self.scale(a[start + j + half], tw[j])
                    a[start + j], a[start + j + half] = self.add(u, t), self.sub(u, t)
            half *= 2
        ni, hi = pow(n, p - 2, p), pow(h, p - 2, p)
        return [self.scale(c, ni * pow(hi, j, p) % p) for j, c in enumerate(a)]

    def verify_query(self, k, h, a, num_folds, roots, betas, final, index, openings):
        """openings[l] = (row stored, path) of row (position mod rows) of layer l; final [d][size] stored"""
        p = self.p
        pos, value = index % (1 << k), None
        for l, al in enumerate(self.layer_arities(k, a, num_folds)):
            m = 1 << (k - al)
            r, j = pos % m, pos // m
            row, path = openings[l]
            if not MR.verify(self.name, roots[l], m, r, list(row), list(path)):
                return False
            elems = [tuple(self.pl(row[(c << al) + jj]) for c in range(self.d)) for jj in range(1 << al)]
            if value is not None and elems[j] != value:
                return False
            # the row as a layer of size 2^al over the coset of its own point: fold it down to one value
            x = h * pow(self.omega(k), r, p) % p
            value = self.fold_row(elems, al, x, k, self.plain(betas[l]))
            k, h, pos = k - al, pow(h, 1 << al, p), r
        if value is None:
            return True
        x = h * pow(self.omega(k), pos, p) % p
        acc = self.zero()
        for i in range(len(final[0]) - 1, -1, -1):
            acc = self.add(self.scale(acc, x), tuple(self.pl(final[c][i]) for c in range(self.d)))
        return acc == value

    def fold_row(self, elems, al, x, k, beta):
        """the 2^al values f(x zeta^j), zeta = w^(n / 2^al), folded to g(x^(2^al)): the evaluation formula on a layer of 2^al"""
        # positions i + j m of the big layer are the size-2^al coset x <zeta> in natural order
        return self._fold_small(elems, al, x, beta)

    def _fold_small(self, f, al, x, beta):
        p = self.p
        for lev in range(al):
            size = 1 << (al - lev)
            z = self.omega(al - lev)
            half = size // 2
            inv2 = pow(2, p - 2, p)
            out = []
            for i in range(half):
                pt = x * pow(z, i, p) % p
                s = self.scale(self.add(f[i], f[i + half]), inv2)
                dlt = self.scale(self.sub(f[i], f[i + half]), pow(2 * pt, p - 2, p))
                out.append(self.add(s, self.mul(beta, dlt)))
            f, x, beta = out, x * x % p, self.mul(beta, beta)
        return f[0]


GOLDILOCKS = ExtField("GOLDILOCKS", 0, 2**64 - 2**32 + 1, 7, 64, 7, 2)
BABYBEAR = ExtField("BABYBEAR", 1, 2**31 - 2**27 + 1, 31, 32, 11, 4)
KOALABEAR = ExtField("KOALABEAR", 2, 2**31 - 2**24 + 1, 3, 32, 3, 4)
FIELDS = {f.name: f for f in (GOLDILOCKS, BABYBEAR, KOALABEAR)}


def rng(seed):
    return random.Random(seed)


def shake_challenge(x, transcript):
    """A challenge function for the commit phase: SHAKE256 of the running roots, d stored residues (rejection-free: 128 bits per
    component reduced mod p)."""
    def fn(root):
        transcript.append(bytes(root))
        out = hashlib.shake_256(b"".join(transcript)).digest(16 * x.d)
        return tuple(int.from_bytes(out[16 * k:16 * k + 16], "little") % x.p for k in range(x.d))
    return fn
