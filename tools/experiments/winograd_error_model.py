"""CPU estimate of the rounding error of the F(2,3)-along-y form of a 3x3 layer (conv_wino.h; conv_cfg.h: Cfg::WINO) against a direct fp32
convolution, both measured against float64: inputs, weights, pre-BN and residual drawn as tests/test_gpu_parity.py draws them, the
four GEMMs as 1x3 fp32 convolutions over the transformed rows.  torch's CPU kernels do not sum in the GPU tile's k order, so these
are estimates of size; the measured figures are tests/test_gpu_winograd.py's (profiles/r08_winograd_error.txt)."""
import numpy as np, torch
torch.set_num_threads(16)
F = torch.nn.functional
def run(cin, cout, size, batch, seed, res=True):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    ps = rs.uniform(0.5, 1.5, cin).astype(np.float32); pt = (rs.standard_normal(cin) * 0.3).astype(np.float32)
    r = rs.standard_normal((batch, cout, size, size)).astype(np.float32)
    xt = torch.from_numpy(x); wt = torch.from_numpy(w)
    a32 = torch.relu(xt * torch.from_numpy(ps)[None, :, None, None] + torch.from_numpy(pt)[None, :, None, None])
    a64 = torch.relu(xt.double() * torch.from_numpy(ps).double()[None, :, None, None] + torch.from_numpy(pt).double()[None, :, None, None])
    want = F.conv2d(a64, wt.double(), None, 1, 1) + (torch.from_numpy(r).double() if res else 0)
    direct = F.conv2d(a32, wt, None, 1, 1) + (torch.from_numpy(r) if res else 0)
    # F(2,3) along y: weights transformed in float64, rounded once to fp32
    g = wt.double()  # [co, ci, ky, kx]
    U = torch.stack([g[:, :, 0], (g[:, :, 0] + g[:, :, 1] + g[:, :, 2]) / 2, (g[:, :, 0] - g[:, :, 1] + g[:, :, 2]) / 2, g[:, :, 2]], 0).float()  # [4, co, ci, kx]
    ap = F.pad(a32, (0, 0, 1, 1))  # zero rows after the activation; x padding is left to the 1x3 conv
    d0, d1, d2, d3 = ap[:, :, 0:size:2], ap[:, :, 1:size + 1:2], ap[:, :, 2:size + 2:2], ap[:, :, 3:size + 3:2]
    V = [d0 - d2, d1 + d2, d2 - d1, d1 - d3]
    M = [F.conv2d(V[t], U[t][:, :, None, :].contiguous(), None, 1, (0, 1)) for t in range(4)]
    even = (M[0] + M[1]) + M[2]
    odd = (M[1] - M[2]) - M[3]
    out = torch.empty_like(direct)
    out[:, :, 0::2] = even; out[:, :, 1::2] = odd
    if res: out = out + torch.from_numpy(r)
    # exact algebra check in float64
    Ud = torch.stack([g[:, :, 0], (g[:, :, 0] + g[:, :, 1] + g[:, :, 2]) / 2, (g[:, :, 0] - g[:, :, 1] + g[:, :, 2]) / 2, g[:, :, 2]], 0)
    apd = F.pad(a64, (0, 0, 1, 1))
    e0, e1, e2, e3 = apd[:, :, 0:size:2], apd[:, :, 1:size + 1:2], apd[:, :, 2:size + 2:2], apd[:, :, 3:size + 3:2]
    Vd = [e0 - e2, e1 + e2, e2 - e1, e1 - e3]
    Md = [F.conv2d(Vd[t], Ud[t][:, :, None, :].contiguous(), None, 1, (0, 1)) for t in range(4)]
    o64 = torch.empty_like(want); o64[:, :, 0::2] = Md[0] + Md[1] + Md[2]; o64[:, :, 1::2] = Md[1] - Md[2] - Md[3]
    if res: o64 = o64 + torch.from_numpy(r).double()
    tol = 5e-6 * max(1.0, want.abs().max().item())
    ed = (direct.double() - want).abs().max().item(); ew = (out.double() - want).abs().max().item()
    print(f"cin {cin} cout {cout} size {size} b {batch}: tol {tol:.2e} direct(torch f32) {ed:.2e} wino-y f32 {ew:.2e} ratio {ew/ed:.2f} wino/tol {ew/tol:.2f} algebra(f64) {(o64-want).abs().max().item():.1e}")
run(256, 256, 32, 2, 1); run(256, 128, 64, 1, 2); run(128, 64, 32, 2, 3); run(256, 128, 128, 2, 4); run(64, 64, 64, 2, 5, res=False)
