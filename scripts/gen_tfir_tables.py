"""Derive the Toom-Cook tables of the stem's temporal fast-FIR schemes (csrc/conv_stem_tfir_f32.hip) exactly, from rational
Vandermonde matrices, and print them as the `static const float` initialisers committed in that file.

    python scripts/gen_tfir_tables.py

F(m, r) on n = m + r - 1 points p_j (the last one is infinity): A^T[o][j] = p_j^o, G[j][k] = p_j^k, B^T = inverse transpose
of the n x n Vandermonde V[j][i] = p_j^i; the infinity row is the leading coefficient ([o == m - 1], [k == r - 1],
[i == n - 1]).  Then  sum_j A^T[o][j] G[j][k] B^T[j][i] == [i == o + k].  A split scheme computes the taps [0, r1) and
[r1, r1 + r2) by two such forms; its tables are the two block-wise (zeros elsewhere), the second block's inputs start at r1.
"""
from fractions import Fraction as Fr

INF = None
KT = 7


def vander(points, cols):
    return [[(Fr(1) if c == cols - 1 else Fr(0)) if p is INF else Fr(p) ** c for c in range(cols)] for p in points]


def inverse(a):
    n = len(a)
    a = [row[:] + [Fr(int(i == j)) for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c] != 0)
        a[c], a[piv] = a[piv], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                a[r] = [v - a[r][c] * w for v, w in zip(a[r], a[c])]
    return [row[n:] for row in a]


def form(m, r, points):
    n = m + r - 1
    assert len(points) == n
    at = [list(col) for col in zip(*vander(points, m))]           # m x n
    g = vander(points, r)                                         # n x r
    inv = inverse(vander(points, n))                              # V^-1; B^T[j][i] = V^-1[i][j]
    bt = [[inv[i][j] for i in range(n)] for j in range(n)]
    return at, g, bt


def scheme(sid):
    """(m, P, A^T m x P, G P x kT, B^T P x (m + kT - 1)) of scheme `sid`, as Fractions."""
    h, q = Fr(1, 2), Fr(1, 4)
    if sid == 1:
        parts = [(2, 7, [0, 1, -1, 2, -2, h, -h, INF])]
    elif sid == 2:
        parts = [(4, 4, [0, 1, -1, 2, -2, h, INF]), (4, 3, [0, 1, -1, 2, -2, INF])]
    elif sid == 3:
        parts = [(4, 7, [0, 1, -1, 2, -2, h, -h, 4, q, INF])]
    else:
        raise ValueError(sid)
    m = parts[0][0]
    P, win = sum(mm + r - 1 for mm, r, _ in parts), m + KT - 1
    AT = [[Fr(0)] * P for _ in range(m)]
    G = [[Fr(0)] * KT for _ in range(P)]
    BT = [[Fr(0)] * win for _ in range(P)]
    j0 = k0 = 0
    for mm, r, pts in parts:
        at, g, bt = form(mm, r, pts)
        n = mm + r - 1
        for j in range(n):
            for o in range(m):
                AT[o][j0 + j] = at[o][j]
            for k in range(r):
                G[j0 + j][k0 + k] = g[j][k]
            for i in range(n):
                BT[j0 + j][k0 + i] = bt[j][i]
        j0, k0 = j0 + n, k0 + r
    assert k0 == KT
    for o in range(m):
        for k in range(KT):
            for i in range(win):
                assert sum(AT[o][j] * G[j][k] * BT[j][i] for j in range(P)) == int(i == o + k)
    return m, P, AT, G, BT


def c_rows(name, mat):
    def lit(v):
        if v.denominator == 1:
            return "%d.f" % v.numerator
        return "%d.f / %d.f" % (v.numerator, v.denominator)
    rows = ",\n".join("    " + ", ".join(lit(v) for v in row) for row in mat)
    return "static const float %s[] = {\n%s};" % (name, rows)


if __name__ == "__main__":
    for sid in (1, 2, 3):
        m, P, AT, G, BT = scheme(sid)
        print("// scheme %d: m = %d, P = %d" % (sid, m, P))
        print(c_rows("kAT%d" % sid, AT))
        print(c_rows("kG%d" % sid, G))
        print(c_rows("kBT%d" % sid, BT))
