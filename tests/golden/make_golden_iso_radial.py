#!/usr/bin/env python3
"""Golden vectors for second-order operators on the ISOTROPIC Matern kernel (the radial family, `LPGP_MATERN_RADIAL`).

  iso_radial.npz
    Kernel blocks.  k(x, x') = kappa_nu(|| a .* (x - x') ||), a = sqrt(2 nu) / lengthscales, differentiated SYMBOLICALLY by SymPy (as a
    function of delta = x - x': d/dx_i = d/ddelta_i, d/dx'_i = -d/ddelta_i) and evaluated in mpmath with at least 50 correct
    digits (the raw derivative of the closed form in the distance cancels like s^-7 near s = 0: the working precision grows with
    -log10 s; coincident points take the one-sided limit along a fixed direction, delta = 1e-45 * e, the limit being
    direction-independent for nu >= 5/2 and at most two derivatives per argument).
      cases      d in {2, 3}  x  nu in {5/2, 7/2, 9/2}, anisotropic lengthscales               tag  d{d}_nu{2 nu}2
      operators  lap_id (Lap, id), id_lap (id, Lap), lap_lap (Lap, Lap), d01_lap (d^2/dx_0 dx_1, Lap),
                 mix_mix (2 id - 0.5 Lap + <v, grad> on both arguments)
      points     24 rows x 24 columns: columns 0-3 coincide with rows 0-3, columns 4-7 / 8-11 lie 1e-9 / 1e-5 of a
                 lengthscale from rows 4-7 / 8-11, columns 12-15 at s ~ 50 from rows 12-15, the rest scattered
      {tag}_{op}    the block,  {tag}_{op}_E  its envelope: the closed form  e^{-s} sum Theta_m(s) Pi_m(u)  (lower.cpp:
                 lower_radial_group) with the absolute value of EVERY summand -- per term of the operator pair, per index j of the
                 expansion of d_u^alpha psi, per power of s in Theta_m.  The closed form itself is checked against SymPy here.
    Posterior.  post_*: 2-D Poisson problem, prior Matern-5/2 (isotropic, anisotropic lengthscales), 64 scattered collocation
      points under -Lap (f = 2 pi^2 sin pi x sin pi y), then 32 boundary values 0 with a 1e-8 nugget, 20 prediction points;
      Gram matrix, Cholesky solve, mean and variance in 50-digit mpmath (as make_golden_multiblock.py).

  iso_first.npz
    First-order operators on the same kernel (the isotropic group of the first-order lowering, `LPGP_MATERN_ISO`: value, directional
    derivative and the mixed u^T B u term), by the same machinery: SymPy derivatives in mpmath, the all-summands-absolute envelope of
    the closed form, the same 24 x 24 planted point layout (an own seed, so that iso_radial.npz does not change).
      cases      d in {2, 3}  x  nu in {3/2, 5/2, 7/2}, anisotropic lengthscales; nu = 1/2 for id_id only, nu = 3/2 without grad_grad
                 and mix (a derivative on both arguments: the lowering refuses it there)                       tag  d{d}_nu{2 nu}2
      operators  id_id, grad_id (<v, grad> on the first argument), id_grad (<w, grad'> on the second), grad_grad (<v, grad>,
                 <w, grad'>, v != w: the matrix B of the mixed term is not symmetric), mix (c + <v, grad> on both arguments)
      {tag}_{op}    the block (float64),  {tag}_{op}_E  its envelope, float32 rounded UP (an upper bound needs no more digits)

Run:  python tests/golden/make_golden_iso_radial.py [iso_radial | iso_first]     (a few minutes each; no argument: both)
"""
import itertools
import os
import sys

import mpmath
import numpy as np
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
mp = mpmath.mp
BASE_DPS = 60


def multi_indices(d, order):
    return [a for a in itertools.product(range(order + 1), repeat=d) if sum(a) <= order]


def matern_poly(p):
    """P_p(s), kappa = e^{-s} P_p(s): sympy polynomial with rational coefficients."""
    s = sp.Symbol("s", positive=True)
    return s, sum(sp.Rational(sp.factorial(2 * p - k), sp.factorial(p - k) * sp.factorial(k)) * 2**k * s**k for k in range(p + 1)) / sp.Rational(sp.factorial(2 * p), sp.factorial(p))


class Kernel:
    """All partial derivatives of f(delta) = kappa(|a .* delta|) up to total order `order`, lambdified for mpmath."""

    def __init__(self, d, p, ls, order=4):
        self.d, self.p = d, p
        self.ls = [sp.Rational(str(l)) for l in ls]
        self.a = [sp.sqrt(2 * p + 1) / l for l in self.ls]
        dl = sp.symbols(f"d0:{d}", real=True)
        s, P = matern_poly(p)
        r = sp.sqrt(sum((a * x) ** 2 for a, x in zip(self.a, dl)))
        f = (P * sp.exp(-s)).subs(s, r)
        self.alphas = multi_indices(d, order)
        cache = {(0,) * d: f}
        for al in sorted(self.alphas, key=sum):
            if al in cache:
                continue
            j = next(i for i in range(d) if al[i] > 0)
            lower = tuple(v - (1 if i == j else 0) for i, v in enumerate(al))
            cache[al] = sp.diff(cache[lower], dl[j])
        self.fn = sp.lambdify(dl, [cache[al] for al in self.alphas], "mpmath", cse=True)
        # closed form: Theta_m as Laurent polynomials {power: rational}
        th = [sp.expand(P)]
        for m in range(4):
            th.append(sp.expand((sp.diff(th[-1], s) - th[-1]) / s))
        self.theta = []
        for t in th:
            co = {}
            for term in sp.Add.make_args(sp.expand(t)):
                c, pw = term.as_coeff_exponent(s)
                co[int(pw)] = co.get(int(pw), 0) + c
            self.theta.append(co)

    def derivs(self, delta):
        """{alpha: d^alpha f(delta)} to 50+ digits; delta a list of mpf (exact differences)."""
        a = [mpmath.mpf(sp.N(x, 80)) for x in self.a]
        s = mpmath.sqrt(sum((ai * di) ** 2 for ai, di in zip(a, delta)))
        if s == 0:
            mp.dps = BASE_DPS + 9 * 45 + 20
            e = [mpmath.mpf(v) for v in (0.6, -0.5, 0.62)[: self.d]]
            vals = self.fn(*[mpmath.mpf(10) ** -45 * v for v in e])
        else:
            mp.dps = BASE_DPS + int(9 * max(0.0, -float(mpmath.log10(s)))) + 10
            vals = self.fn(*delta)
        vals = [+v for v in vals]
        mp.dps = BASE_DPS
        return dict(zip(self.alphas, vals))

    def closed_form(self, delta, terms):
        """(value, envelope) of sum_t c_t d^{n0} d'^{n1} k from the radial closed form, in mpmath."""
        mp.dps = BASE_DPS
        a = [mpmath.mpf(sp.N(x, 80)) for x in self.a]
        u = [ai * di for ai, di in zip(a, delta)]
        s = mpmath.sqrt(sum(v * v for v in u))
        val, env = mpmath.mpf(0), mpmath.mpf(0)
        for c, n0, n1 in terms:
            al = tuple(x + y for x, y in zip(n0, n1))
            pref = mpmath.mpf(c) * (-1) ** sum(n1)
            for ai, k in zip(a, al):
                pref *= ai**k
            for jj in itertools.product(*[range(k // 2 + 1) for k in al]):
                w = pref
                mono = mpmath.mpf(1)
                for k, j, uu in zip(al, jj, u):
                    w *= mpmath.factorial(k) / (mpmath.factorial(j) * mpmath.factorial(k - 2 * j) * 2**j)
                    mono *= uu ** (k - 2 * j)
                m = sum(al) - sum(jj)
                for pw, co in self.theta[m].items():
                    if pw < 0 and s == 0:
                        assert mono == 0
                        continue
                    t = w * mono * mpmath.mpf(sp.N(co, 80)) * s**pw * mpmath.exp(-s)
                    val += t
                    env += abs(t)
        return val, env


def operator_pairs(d):
    z = (0,) * d

    def e(i, k=1):
        return tuple(k if j == i else 0 for j in range(d))

    ident = {z: 1.0}
    lap = {e(i, 2): 1.0 for i in range(d)}
    d01 = {tuple(1 if j < 2 else 0 for j in range(d)): 1.0}
    v = (0.7, -0.4, 0.3)[:d]
    mix = {z: 2.0}
    for i in range(d):
        mix[e(i, 2)] = -0.5
        mix[e(i)] = v[i]
    return {"lap_id": (lap, ident), "id_lap": (ident, lap), "lap_lap": (lap, lap), "d01_lap": (d01, lap), "mix_mix": (mix, mix)}, v


def term_list(L0, L1):
    return [(c0 * c1, a, b) for a, c0 in L0.items() for b, c1 in L1.items()]


def points(d, p, ls, rng):
    ls = np.asarray(ls)
    X0 = rng.uniform(-1.0, 1.0, size=(24, d))
    X1 = rng.uniform(-1.0, 1.0, size=(24, d))
    X1[0:4] = X0[0:4]
    for i in range(4, 8):
        e = rng.normal(size=d)
        X1[i] = X0[i] + 1e-9 * ls * e / np.linalg.norm(e)
    for i in range(8, 12):
        e = rng.normal(size=d)
        X1[i] = X0[i] + 1e-5 * ls * e / np.linalg.norm(e)
    for i in range(12, 16):
        e = rng.normal(size=d)
        X1[i] = X0[i] + 50.0 / np.sqrt(2 * p + 1) * ls * e / np.linalg.norm(e)
    return X0, X1


def mpf_delta(x, y):
    return [mpmath.mpf(float(a)) - mpmath.mpf(float(b)) for a, b in zip(x, y)]


def kernel_case(d, p, ls, rng, out):
    tag = f"d{d}_nu{2 * p + 1}2"
    K = Kernel(d, p, ls)
    ops, v = operator_pairs(d)
    X0, X1 = points(d, p, ls, rng)
    out[f"{tag}_X0"], out[f"{tag}_X1"], out[f"{tag}_lengthscales"], out[f"{tag}_v"] = X0, X1, np.asarray(ls, dtype=float), np.asarray(v)
    blocks = {name: (np.zeros((24, 24)), np.zeros((24, 24))) for name in ops}
    worst = 0.0
    for i in range(24):
        for j in range(24):
            dl = mpf_delta(X0[i], X1[j])
            D = K.derivs(dl)
            for name, (L0, L1) in ops.items():
                terms = term_list(L0, L1)
                g = sum(mpmath.mpf(c) * (-1) ** sum(b) * D[tuple(x + y for x, y in zip(a, b))] for c, a, b in terms)
                cv, env = K.closed_form(dl, terms)
                if env == 0:                     # (every summand vanishes at coincident points, e.g. odd mixed derivatives: the limit is 0)
                    assert abs(g) < mpmath.mpf(10) ** -40, g
                    g = mpmath.mpf(0)
                else:
                    worst = max(worst, float(abs(g - cv) / env))
                blocks[name][0][i, j] = float(g)
                blocks[name][1][i, j] = float(env)
    assert worst < 1e-40, worst         # the closed form IS the symbolic derivative
    for name, (G, E) in blocks.items():
        out[f"{tag}_{name}"], out[f"{tag}_{name}_E"] = G, E
    print(f"{tag}: closed form vs SymPy, worst |diff| / E = {worst:.1e}", flush=True)


def first_order_pairs(d):
    z = (0,) * d

    def e(i):
        return tuple(1 if j == i else 0 for j in range(d))

    v, w, c = (0.7, -0.4, 0.3)[:d], (-0.5, 0.9, 0.6)[:d], 1.5
    ident = {z: 1.0}
    gv, gw = {e(i): v[i] for i in range(d)}, {e(i): w[i] for i in range(d)}
    mix = dict(gv)
    mix[z] = c
    return {"id_id": (ident, ident), "grad_id": (gv, ident), "id_grad": (ident, gw), "grad_grad": (gv, gw), "mix": (mix, mix)}, v, w, c


def first_order_case(d, p, ls, rng, out):
    """One (d, nu) case of iso_first.npz; nu = 1/2 (p = 0) is not differentiable: id_id only."""
    tag = f"d{d}_nu{2 * p + 1}2"
    K = Kernel(d, p, ls, order=2 if p else 0)
    ops, v, w, c = first_order_pairs(d)
    if p == 0:
        ops = {"id_id": ops["id_id"]}
    elif p == 1:                         # (the library admits p derivatives in all on the multivariate kernel, as the reference does)
        ops = {name: ops[name] for name in ("id_id", "grad_id", "id_grad")}
    X0, X1 = points(d, p, ls, rng)
    out[f"{tag}_X0"], out[f"{tag}_X1"], out[f"{tag}_lengthscales"] = X0, X1, np.asarray(ls, dtype=float)
    out[f"{tag}_v"], out[f"{tag}_w"], out[f"{tag}_c"] = np.asarray(v), np.asarray(w), c
    blocks = {name: (np.zeros((24, 24)), np.zeros((24, 24), dtype=np.float32)) for name in ops}
    worst = 0.0
    for i in range(24):
        for j in range(24):
            dl = mpf_delta(X0[i], X1[j])
            D = K.derivs(dl)
            for name, (L0, L1) in ops.items():
                terms = term_list(L0, L1)
                g = sum(mpmath.mpf(c0) * (-1) ** sum(b) * D[tuple(x + y for x, y in zip(a, b))] for c0, a, b in terms)
                cv, env = K.closed_form(dl, terms)
                if env == 0:                     # (a directional derivative at coincident points: every summand vanishes)
                    assert abs(g) < mpmath.mpf(10) ** -40, g
                    g = mpmath.mpf(0)
                else:
                    worst = max(worst, float(abs(g - cv) / env))
                blocks[name][0][i, j] = float(g)
                e32 = np.float32(float(env))
                blocks[name][1][i, j] = e32 if mpmath.mpf(float(e32)) >= env else np.nextafter(e32, np.float32(np.inf))
    assert worst < 1e-40, worst
    for name, (G, E) in blocks.items():
        assert np.all(np.abs(G) <= E.astype(np.double))
        out[f"{tag}_{name}"], out[f"{tag}_{name}_E"] = G, E
    print(f"{tag} (first order): closed form vs SymPy, worst |diff| / E = {worst:.1e}", flush=True)


def posterior(out):
    d, p, ls, scale = 2, 2, (0.6, 0.5), 1.5
    K = Kernel(d, p, ls)
    rng = np.random.default_rng(20241018)
    Xc = rng.uniform(-0.95, 0.95, size=(64, 2))
    t = (np.arange(8) + 0.5) / 8 * 2 - 1
    Xb = np.concatenate([np.column_stack([np.full(8, -1.0), t]), np.column_stack([np.full(8, 1.0), t]),
                         np.column_stack([t, np.full(8, -1.0)]), np.column_stack([t, np.full(8, 1.0)])])
    Xt = rng.uniform(-0.9, 0.9, size=(20, 2))
    Yc = 2 * np.pi**2 * np.sin(np.pi * Xc[:, 0]) * np.sin(np.pi * Xc[:, 1])
    Yb = np.zeros(32)
    ident, mlap = {(0, 0): 1.0}, {(2, 0): -1.0, (0, 2): -1.0}
    Xs, Ls, ys, noises = [Xc, Xb], [mlap, ident], [Yc, Yb], ["0", "1e-8"]

    def entry(L0, L1, x, y):
        D = K.derivs(mpf_delta(x, y))
        return scale * sum(mpmath.mpf(c) * (-1) ** sum(b) * D[tuple(u + w for u, w in zip(a, b))] for c, a, b in term_list(L0, L1))

    N = 96
    Xall = np.concatenate(Xs)
    Lall = [Ls[0]] * 64 + [Ls[1]] * 32
    G = mpmath.zeros(N, N)
    for i in range(N):
        for j in range(i + 1):
            G[i, j] = entry(Lall[i], Lall[j], Xall[i], Xall[j])
            G[j, i] = G[i, j]
    for i in range(64, 96):
        G[i, i] += mpmath.mpf(noises[1])
    mp.dps = 50
    C = mpmath.cholesky(G)

    def solve(b):
        z = mpmath.matrix(N, 1)
        for i in range(N):
            z[i] = (b[i] - sum(C[i, k] * z[k] for k in range(i))) / C[i, i]
        return z

    def solve_t(z):
        w = mpmath.matrix(N, 1)
        for i in reversed(range(N)):
            w[i] = (z[i] - sum(C[k, i] * w[k] for k in range(i + 1, N))) / C[i, i]
        return w

    y = mpmath.matrix([mpmath.mpf(float(v)) for v in np.concatenate(ys)])
    w = solve_t(solve(y))
    mean, var = [], []
    for x in Xt:
        krow = mpmath.matrix([entry(ident, Lall[i], x, Xall[i]) for i in range(N)])
        mean.append(float(sum(krow[i] * w[i] for i in range(N))))
        z = solve(krow)
        var.append(float(mpmath.mpf(scale) - sum(z[i] * z[i] for i in range(N))))
    Gf = np.array([[float(G[i, j]) for j in range(N)] for i in range(N)])
    cond = float(np.linalg.cond(Gf))
    out.update({"post_Xc": Xc, "post_Xb": Xb, "post_Xt": Xt, "post_Yc": Yc, "post_Yb": Yb, "post_lengthscales": np.asarray(ls), "post_scale": scale,
                "post_nugget": 1e-8, "post_weights": np.array([float(v) for v in w]), "post_mean": np.array(mean), "post_var": np.array(var),
                "post_cond": cond})
    print(f"posterior: N = {N}, cond_2(G) = {cond:.2e}", flush=True)


def main_radial():
    out = {}
    rng = np.random.default_rng(20241017)
    for d, ls in ((2, (0.9, 0.6)), (3, (0.9, 0.6, 1.3))):
        for p in (2, 3, 4):
            kernel_case(d, p, ls, rng, out)
    posterior(out)
    path = os.path.join(HERE, "iso_radial.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


def main_first():
    out = {}
    rng = np.random.default_rng(20241019)
    for d, ls in ((2, (0.9, 0.6)), (3, (0.9, 0.6, 1.3))):
        for p in (0, 1, 2, 3):
            first_order_case(d, p, ls, rng, out)
    path = os.path.join(HERE, "iso_first.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "iso_radial.npz"))


def main():
    which = sys.argv[1:] or ["iso_radial", "iso_first"]
    if "iso_radial" in which:
        main_radial()
    if "iso_first" in which:
        main_first()


if __name__ == "__main__":
    sys.exit(main())
