"""CPU model of the rounding error of a 3x3 layer as the direct tile, as F(2,3) along y (conv_wino.h; conv_cfg.h: Cfg::WINO) and as F(4,3) along
y (Cfg::WINO4) on two point sets, each against float64.

The model is the tiles' arithmetic: BatchNorm + ReLU in fp32, the input transform in fp32 summed left to right (all coefficients
are dyadic: the products are exact), weights transformed in float64 and rounded once, one sequential fp32 accumulation chain per
output and GEMM in the tiles' k order (4-channel chunk, tap or kx, channel), the output transform in fp32.  A product of two fp32
values is exact in float64, so a chain step is float32(float64(acc) + a * b).  Standard-normal inputs, weights / sqrt(9 cin).

    python tools/experiments/winograd4_error_model.py

prints, per (cin, cout, size), the largest error of each form, its ratio to the direct form's and its share of the single-layer
bound 5e-6 * max(1, |want|max) of tests/test_gpu_parity.py::test_conv2d_matches_torch."""
import numpy as np

F32 = np.float32

# transforms as (BT [t, rows in], G [t, 3], AT [rows out, t])
F23 = (np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float),
       np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
       np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float))
# points 0, 1, -1, 2, -2, inf (the textbook set)
F43_TEXTBOOK = (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], float),
                np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
                np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float))
# points 0, 1, -1, 2, -1/2, inf (the tile's)
F43_TILE = (np.array([[1, 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -.5, 1, 0], [0, 1, .5, -2.5, 1, 0], [0, -.5, -1, .5, 1, 0], [0, 2, -1, -2, 1, 0], [0, 1, 1.5, -2, -1.5, 1]]),
            np.array([[1, 0, 0], [-1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3], [1 / 15, 2 / 15, 4 / 15], [-16 / 15, 8 / 15, -4 / 15], [0, 0, 1]]),
            np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -.5, 0], [0, 1, 1, 4, .25, 0], [0, 1, -1, 8, -.125, 1]]))


def chain(acc, a, b):
    """acc [cout, ...] += a [cout] (x) b [...], one fp32 rounding"""
    return (acc.astype(np.float64) + a.astype(np.float64).reshape((-1,) + (1,) * b.ndim) * b.astype(np.float64)).astype(F32)


def lin32(coef, rows):
    """sum_j coef[j] rows[j] in fp32, left to right, zero coefficients skipped"""
    out = None
    for c, r in zip(coef, rows):
        if c != 0:
            term = (F32(c) * r).astype(F32)
            out = term if out is None else (out + term).astype(F32)
    return out


def direct32(a, w):
    cin, H, W = a.shape
    ap = np.zeros((cin, H + 2, W + 2), F32)
    ap[:, 1:-1, 1:-1] = a
    acc = np.zeros((w.shape[0], H, W), F32)
    for cb in range(0, cin, 4):
        for ky in range(3):
            for kx in range(3):
                for c in range(cb, min(cb + 4, cin)):
                    acc = chain(acc, w[:, c, ky, kx], ap[c, ky:ky + H, kx:kx + W])
    return acc


def winograd32(a, w, form):
    BT, G, AT = form
    nt, rows_in = BT.shape
    rows_out = AT.shape[0]
    cin, H, W = a.shape
    ap = np.zeros((cin, H + 2, W + 2), F32)
    ap[:, 1:-1, 1:-1] = a
    u = np.einsum("tk,ockx->tocx", G, w.astype(np.float64)).astype(F32)  # [t, cout, cin, kx], one rounding
    out = np.zeros((w.shape[0], H, W), F32)
    for q in range(H // rows_out):
        d = [ap[:, rows_out * q + r] for r in range(rows_in)]  # [cin, W + 2] each
        v = [lin32(BT[t], d) for t in range(nt)]
        m = [np.zeros((w.shape[0], W), F32) for _ in range(nt)]
        for cb in range(0, cin, 4):
            for kx in range(3):
                for c in range(cb, min(cb + 4, cin)):
                    for t in range(nt):
                        m[t] = chain(m[t], u[t, :, c, kx], v[t][c, kx:kx + W])
        for r in range(rows_out):
            out[:, rows_out * q + r] = lin32(AT[r], m)
    return out


def run(cin, cout, size, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((cin, size, size)).astype(F32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(F32)
    ps, pt = rs.uniform(0.5, 1.5, cin).astype(F32), (rs.standard_normal(cin) * 0.3).astype(F32)
    a32 = np.maximum(x * ps[:, None, None] + pt[:, None, None], F32(0)).astype(F32)
    a64 = np.maximum(x.astype(np.float64) * ps[:, None, None] + pt[:, None, None].astype(np.float64), 0.0)
    ap = np.zeros((cin, size + 2, size + 2))
    ap[:, 1:-1, 1:-1] = a64
    want = np.zeros((cout, size, size))
    for ky in range(3):
        for kx in range(3):
            want += np.einsum("oc,cyx->oyx", w[:, :, ky, kx].astype(np.float64), ap[:, ky:ky + size, kx:kx + size])
    tol = 5e-6 * max(1.0, np.abs(want).max())
    ed = np.abs(direct32(a32, w) - want).max()
    line = f"{cin:3d}->{cout} @{size}: bound {tol:.2e}  direct {ed:.2e} ({ed / tol:.2f} of the bound)"
    for name, form in (("F(2,3)", F23), ("F(4,3) 0,+-1,+-2,inf", F43_TEXTBOOK), ("F(4,3) 0,1,-1,2,-1/2,inf", F43_TILE)):
        e = np.abs(winograd32(a32, w, form) - want).max()
        line += f"  {name} {e:.2e} = {e / ed:.2f}x direct, {e / tol:.2f} of the bound"
    print(line, flush=True)


if __name__ == "__main__":
    for form in (F23, F43_TEXTBOOK, F43_TILE):  # the algebra: AT [(G g) * (BT d)] is the correlation of d with g
        rs = np.random.RandomState(1)
        g, d = rs.standard_normal(3), rs.standard_normal(form[0].shape[1])
        ref = np.array([d[i:i + 3] @ g for i in range(form[2].shape[0])])
        assert np.abs(form[2] @ ((form[1] @ g) * (form[0] @ d)) - ref).max() < 1e-13
    run(256, 32, 16, 1)
    run(128, 32, 16, 2)
    run(76, 32, 16, 3)
