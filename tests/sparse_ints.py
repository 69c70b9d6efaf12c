"""Dense-by-sparse negacyclic products in Python integers: what makes a whole he_mul / he_swk / gemv_inner call exact at a full-size ring
(tests/test_he_mul_full_gpu.py, tests/test_ring15_calls_gpu.py) -- one operand of every polynomial product has a handful of terms."""


def sparse_mul(dense, terms, n):
    """dense * sum(c X^k for k, c in terms) in Z[X] / (X^n + 1), not reduced"""
    out = [0] * n
    for k, c in terms:
        for i, v in enumerate(dense):
            j = i + k
            if j < n:
                out[j] += c * v
            else:
                out[j - n] -= c * v
    return out


def sparse_terms(rng, n, cnt, lim):
    """up to `cnt` terms (k, c) at distinct random positions, c in [-lim, lim), sorted by position"""
    return sorted({rng.randrange(n): rng.randrange(-lim, lim) for _ in range(cnt)}.items())


def dense_of(terms, n):
    d = dict(terms)
    return [d.get(i, 0) for i in range(n)]
