#!/usr/bin/env python3
"""CPU probe of the screened E-step's bound (numpy only; DESIGN.md section 3.3p, device/em_screen_bound.hpp): a numpy EM on 32 768
rows in which every pass after the first applies the screen exactly as the kernel does -- four constants per component from the
block's parameter set and the new one, lw'_ub = alpha lw + A and lw'_lb = alpha' lw + A' on the STORED values, Lmax over the
entries marked exact, candidate unless lw'_ub < Lmax - 746, non-candidates keep their upper bound and lose their exact mark -- and
compares with the dense evaluation of the same pass. Per pass: max f = |I - W' L|_F and max gamma = |W' (mu - mu')| over the
components, candidates per sample, exactly nonzero responsibilities per sample, and MISSED pairs (nonzero but not a candidate:
must be 0). Three fits: the benchmark's mixture from the benchmark's start, the same from means perturbed by 1.5 sigma, and an
overlapping mixture (the same rows with the component means drawn together), where every pair stays a candidate and the runtime's
rule (at most 16 candidates per sample) gives the screen up.

    python tools/estep_screen_probe.py > profiles/estep_screen_probe.txt
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("synth", os.path.join(HERE, "..", "ml_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)

D, K, N, PASSES = 32, 64, 32768, 8
OUT = 2.0 ** -40
MARGIN, MAX_STORED, MAX_PAIRS = 746.0, 2.0 ** 40, 16.0


def factors(S):
    L = np.linalg.cholesky(S)
    return L, np.linalg.inv(L)


def dense(X, pi, mu, W, L):
    lw = np.empty((len(X), K))
    with np.errstate(divide="ignore"):
        coef = np.log(pi) - np.log(np.diagonal(L, axis1=1, axis2=2)).sum(1)
    for k in range(K):
        y = (X - mu[k]) @ W[k].T
        lw[:, k] = coef[k] - 0.5 * (y * y).sum(1)
    return lw, coef


def constants(mu, L, coef, mu2, W2, coef2):
    """(alpha, A, alpha', A') per component, rounded outward like em_screen_bound.hpp; 'no information' -> (0, inf, 0, -inf)."""
    out = np.empty((K, 4))
    fs, gs = np.empty(K), np.empty(K)
    for k in range(K):
        M = W2[k] @ L[k]
        w = np.abs(np.diagonal(L[k]))                                   # (1 / the diagonal of W: the same ratio)
        f = (np.linalg.norm(np.eye(D) - M) * (1 + OUT) + OUT * np.sqrt(D) * (1 + np.linalg.norm(M))
             + D * 2.0 ** -50 * (w.max() / w.min()) * (1 + np.linalg.norm(M)))
        g = np.linalg.norm(W2[k] @ (mu[k] - mu2[k])) * (1 + OUT)
        fs[k], gs[k] = f, g
        a, b = (1 - f) * (1 - OUT), (1 + f) * (1 + OUT)
        ok = np.isfinite([f, g, coef[k], coef2[k]]).all() and a > g
        if not ok:
            out[k] = 0.0, np.inf, 0.0, -np.inf
            continue
        al, al2 = a * (a - g) * (1 - 4 * OUT), b * (b + g) * (1 + 4 * OUT)
        ag, bg = 0.5 * a * g * (1 + OUT), 0.5 * (b * g + g * g) * (1 + 4 * OUT)
        pad = 4 * OUT * (abs(coef2[k]) + al * abs(coef[k]) + ag + 1), 4 * OUT * (abs(coef2[k]) + al2 * abs(coef[k]) + bg + 1)
        out[k] = al, coef2[k] - al * coef[k] + ag + pad[0], al2, coef2[k] - al2 * coef[k] - bg - pad[1]
    return out, fs, gs


def fit(name, X, mu):
    print(f"# {name}")
    print("pass  max_f      max_gamma  no_info  candidates/sample  nonzero/sample  missed  route")
    pi = np.full(K, 1.0 / K)
    S = np.stack([np.cov(X.T)] * K)
    L, W = factors(S)
    stored, coef = dense(X, pi, mu, W, L)              # pass 1 runs dense: there is no block to start from
    exact = np.ones((N, K), bool)
    for t in range(2, PASSES + 2):
        m = stored.max(1, keepdims=True)               # (the statistics pass on the stored block: non-candidates give exactly 0)
        r = np.exp(stored - m)
        r /= r.sum(1, keepdims=True)
        nk = r.sum(0)
        pi2, mu2 = nk / N, (r.T @ X) / nk[:, None]
        S2 = np.empty_like(S)
        for k in range(K):
            Z = X - mu2[k]
            S2[k] = (Z.T * r[:, k]) @ Z / nk[k] + 1e-15 * np.eye(D)
        L2, W2 = factors(S2)
        truth, coef2 = dense(X, pi2, mu2, W2, L2)
        nonzero = np.exp(truth - truth.max(1, keepdims=True)) != 0
        c, fs, gs = constants(mu, L, coef, mu2, W2, coef2)
        no_info = int(np.isinf(c[:, 1]).sum())
        usable = np.abs(stored) < MAX_STORED
        with np.errstate(invalid="ignore"):
            ub, lb = c[:, 0] * stored + c[:, 1], c[:, 2] * stored + c[:, 3]
            lb = np.where(exact & usable, lb, -np.inf)
            Lmax, kmax = lb.max(1, keepdims=True), lb.argmax(1)
            cand = ~(ub < Lmax - MARGIN) | ~usable
        cand[np.arange(N), kmax] = True
        missed = int((nonzero & ~cand).sum())
        per_sample = cand.sum() / N
        route = "dense (no information)" if no_info else "screened" if per_sample <= MAX_PAIRS else "screened; the rule gives it up from here"
        print(f"{t:4d}  {fs.max():.3e}  {gs.max():.3e}  {no_info:7d}  {per_sample:17.2f}  {nonzero.sum() / N:14.2f}  {missed:6d}  {route}")
        if no_info:
            stored, exact = truth, np.ones((N, K), bool)
        else:
            stored, exact = np.where(cand, truth, ub), cand
        pi, mu, S, L, W, coef = pi2, mu2, S2, L2, W2, coef2
    print()


def main():
    mix = synth.Mixture(D, K)
    X, labels = mix.sample(N, stream=0)
    fit("benchmark mixture, benchmark start (true means + 0.5 sigma)", X, mix.initial_means().copy())
    rng = np.random.default_rng(11)
    fit("benchmark mixture, means perturbed by 1.5 sigma", X, mix.means + 1.5 * rng.standard_normal((K, D)))
    near = X - 0.85 * mix.means[labels]
    fit("overlapping mixture (component means drawn together to 0.15 of their distance)", near, 0.15 * mix.initial_means())


if __name__ == "__main__":
    main()
