"""CPU model of the Winograd F(3x3,2x2) scheme of csrc/conv_wino2.hip for the 4x4 stride-2 pad-1 layers (ConvBlock k4 s2
and ConvTBlock of AutoEncoder_DtoD, AE_model_unet.py:497-520): the polyphase decomposition, both tilings (form A: 3x3
tiles of the small image; form B: 6x6 blocks of the large image at offset -1 from one 4x4 patch of the small one), the
role swaps of the two backward passes and the weight gradient, written with the SAME index arithmetic as the kernels and
checked against torch's conv2d / conv_transpose2d autograd.  Pins the transform matrices (F(3,2): points 0, +-1, inf)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _mm(a, b):
    """Batched matrix product on contiguous copies (BLAS)."""
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))).numpy()


def _es(spec, *ops):
    """einsum through torch (pairwise BLAS contractions): the models also run at the GPU tests' channel counts."""
    return torch.einsum(spec, *[torch.from_numpy(np.ascontiguousarray(o)) for o in ops]).numpy()


BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], np.float64)
G = np.array([[1, 0], [.5, .5], [.5, -.5], [0, 1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], np.float64)


def _mats(mats, dtype):
    """(B^T, G, A^T) in dtype: the scheme's own unless given (tests/int_conv_ref.py runs the model on their absolute values)."""
    return [m.astype(dtype) for m in (mats or (BT, G, AT))]


def test_f32_matrices_1d():
    rng = np.random.default_rng(0)
    d, g, dy = rng.standard_normal(4), rng.standard_normal(2), rng.standard_normal(3)
    np.testing.assert_allclose(AT @ ((G @ g) * (BT @ d)), [d[i] * g[0] + d[i + 1] * g[1] for i in range(3)], atol=1e-12)
    np.testing.assert_allclose(G.T @ ((BT @ d) * (AT.T @ dy)), [sum(dy[i] * d[i + u] for i in range(3)) for u in range(2)], atol=1e-12)


def _pad1(x, reflect, dtype):
    C, H, W = x.shape
    if reflect:
        return np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="reflect").astype(dtype)
    xp = np.zeros((C, H + 2, W + 2), dtype)
    xp[:, 1:-1, 1:-1] = x
    return xp


def form_a_input(x, reflect, dtype=np.float64, mats=None):
    """V[16][tile][(a*2+b)*C + c] for the LARGE image x [C,H,W]; tiles of 3x3 outputs = 8x8 footprints at (6t - 1)."""
    bt = _mats(mats, dtype)[0]
    C, H, W = x.shape
    Hy, Wy = H // 2, W // 2
    ty, tx = -(-Hy // 3), -(-Wy // 3)
    xp = _pad1(x, reflect, dtype)                           # xp[r] = x[r - 1]
    big = np.zeros((C, 6 * ty + 2, 6 * tx + 2), dtype)       # rows beyond the padded image read as zero
    big[:, :min(H + 2, big.shape[1]), :min(W + 2, big.shape[2])] = xp[:, :big.shape[1], :big.shape[2]]
    V = np.zeros((4, 4, ty * tx, 4 * C), dtype)
    for t in range(ty * tx):
        a0, b0 = 6 * (t // tx), 6 * (t % tx)
        P = big[:, a0:a0 + 8, b0:b0 + 8]
        for a in range(2):
            for b in range(2):
                X = P[:, a::2, b::2]                          # X_ab[p][q] = P[2p + a][2q + b]
                V[:, :, t, (a * 2 + b) * C:(a * 2 + b + 1) * C] = _es("ij,cjk,lk->ilc", bt, X, bt)
    return V, ty, tx


def form_a_weights(w, dtype=np.float64, mats=None):
    """U[16][n][(a*2+b)*C + c] from w[n][c][4][4] (conv form)."""
    gm = _mats(mats, dtype)[1]
    N, C = w.shape[:2]
    U = np.zeros((4, 4, N, 4 * C), dtype)
    for a in range(2):
        for b in range(2):
            g = w[:, :, a::2, b::2].astype(dtype)            # g_ab[u][v] = w[2u + a][2v + b]
            U[:, :, :, (a * 2 + b) * C:(a * 2 + b + 1) * C] = _es("ij,ncjk,lk->ilnc", gm, g, gm)
    return U


def form_a_output(M, ty, tx, Hy, Wy, keep=None, mats=None):
    """M[16][tile][n] -> y[n][Hy][Wy]."""
    at = _mats(mats, M.dtype)[2]
    y9 = _es("ij,jktn,lk->tnil", at, M, at)                                 # [T,N,3,3]
    y = y9.reshape(ty, tx, -1, 3, 3).transpose(2, 0, 3, 1, 4).reshape(-1, 3 * ty, 3 * tx)
    if keep is not None:
        keep.update(M=M, Y=y)
    return y[:, :Hy, :Wy]


def strided_conv(x, w, reflect, dtype=np.float64, keep=None, mats=None):
    """y = conv2d(pad1(x), w, stride 2) through form A.  Returns y and V.  keep: a dict that receives every intermediate
    (tests/int_conv_ref.py: the exactness bound runs the scheme with mats = the absolute values of BT / G / AT)."""
    V, ty, tx = form_a_input(x, reflect, dtype, mats)
    U = form_a_weights(w, dtype, mats)
    M = _mm(V, U.swapaxes(2, 3)).astype(dtype)
    if keep is not None:
        keep.update(V=V, U=U)
    return form_a_output(M, ty, tx, x.shape[1] // 2, x.shape[2] // 2, keep, mats), V


def transposed_conv(d, wt, Hout, Wout, off, dtype=np.float64, keep=None, mats=None):
    """z[r][s] = sum_{i,j} d[i][j] * wt[:, :, r + 1 - 2i, s + 1 - 2j] through form B; wt[cd][n][4][4].
    off = 0: rows r in [0, Hout);  off = 1: the padded domain, out row = r + 1 for r in [-1, Hout - 2].
    (All tiles at once: one transform of the 4x4 patches, one product per output phase.)"""
    bt, gm, at = _mats(mats, dtype)
    Cd, Hy, Wy = d.shape
    N = wt.shape[1]
    ty, tx = -(-(Hout + 1 - off) // 6), -(-(Wout + 1 - off) // 6)   # = cdiv(Hx + ext, 6): Hx = Hout - 2*off, ext = 1 + off
    dp = np.zeros((Cd, 3 * ty + 3, 3 * tx + 3), dtype)               # dp[s] = d[s - 1]
    dp[:, 1:Hy + 1, 1:Wy + 1] = d
    out = np.zeros((N, Hout, Wout), dtype)
    pat = np.stack([dp[:, 3 * a:3 * a + 4, 3 * b:3 * b + 4] for a in range(ty) for b in range(tx)])          # [T,Cd,4,4]
    Vd = _es("ij,tcjk,lk->iltc", bt, pat, bt)
    big, Us = 0.0, []
    for a in range(2):
        for b in range(2):
            g = np.stack([[wt[:, :, 3 - a - 2 * u, 3 - b - 2 * v] for v in range(2)] for u in range(2)])   # [2,2,cd,n]
            Ug = _es("ij,jkcn,lk->ilcn", gm, g.astype(dtype), gm)
            m = _mm(Vd, Ug).astype(dtype)
            o = _es("ij,jktn,lk->tnil", at, m, at).reshape(ty, tx, N, 3, 3)
            big = max(big, float(np.abs(m).max()), float(np.abs(o).max()))
            Us.append(Ug)
            for i in range(3):
                for j in range(3):
                    oy, ox = 6 * np.arange(ty) + 2 * i - a + off, 6 * np.arange(tx) + 2 * j - b + off
                    vy, vx = (oy >= 0) & (oy < Hout), (ox >= 0) & (ox < Wout)
                    out[np.ix_(np.arange(N), oy[vy], ox[vx])] = o[vy][:, vx][..., i, j].transpose(2, 0, 1)
    if keep is not None:
        keep.update(V=Vd, Us=Us, big=big)
    return out


def lift(sm, ty, tx, dtype=np.float64, mats=None):
    """Dv[16][tile][n] = A s A^T of the 3x3 tiles of the small image."""
    N, Hy, Wy = sm.shape
    gp = np.zeros((N, 3 * ty, 3 * tx), dtype)
    gp[:, :Hy, :Wy] = sm
    g9 = gp.reshape(N, ty, 3, tx, 3).transpose(1, 3, 0, 2, 4).reshape(ty * tx, N, 3, 3)
    at = _mats(mats, dtype)[2]
    return _es("ji,tnjk,kl->iltn", at, g9, at)


def wgrad(V, sm, C, dtype=np.float64, keep=None, P0=None, mats=None):
    """dw[n][c][4][4] from V (form A of the large image) and the small image sm [N,Hy,Wy].
    P0: the per-bin sums of the images before this one (a batch reduces over all its tiles before the tap fold)."""
    Hy, Wy = sm.shape[1:]
    ty, tx = -(-Hy // 3), -(-Wy // 3)
    Dv = lift(sm, ty, tx, dtype, mats)
    gm = _mats(mats, dtype)[1]
    P = _mm(Dv.swapaxes(2, 3), V.astype(dtype)).astype(dtype)
    if P0 is not None:
        P = P + P0
    if keep is not None:
        keep.update(Dv=Dv, P=P)
    dw = np.zeros((sm.shape[0], C, 4, 4), dtype)
    for a in range(2):
        for b in range(2):
            dw[:, :, a::2, b::2] = _es("ji,jknc,kl->ncil", gm, P[:, :, :, (a * 2 + b) * C:(a * 2 + b + 1) * C], gm)
    return dw


def fold_reflect1(dxp):
    """padded-domain gradient [C,H+2,W+2] -> [C,H,W] (rows -1 / H mirror rows 1 / H-2)."""
    g = dxp[:, 1:-1, 1:-1].copy()
    g[:, 1, :] += dxp[:, 0, 1:-1]; g[:, -2, :] += dxp[:, -1, 1:-1]
    g[:, :, 1] += dxp[:, 1:-1, 0]; g[:, :, -2] += dxp[:, 1:-1, -1]
    g[:, 1, 1] += dxp[:, 0, 0]; g[:, 1, -2] += dxp[:, 0, -1]; g[:, -2, 1] += dxp[:, -1, 0]; g[:, -2, -2] += dxp[:, -1, -1]
    return g


@pytest.mark.parametrize("C,N,H,W,reflect", [(3, 2, 12, 18, True), (2, 3, 8, 26, False), (2, 2, 4, 6, True), (1, 2, 16, 10, True),
                                             (2, 1, 14, 4, False)])
def test_strided_conv_all_three_passes(C, N, H, W, reflect):
    rng = np.random.default_rng(H * 100 + W)
    x, w = rng.standard_normal((C, H, W)), rng.standard_normal((N, C, 4, 4))
    gy = rng.standard_normal((N, H // 2, W // 2))
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    xp = F.pad(xt[None], (1, 1, 1, 1), mode="reflect") if reflect else F.pad(xt[None], (1, 1, 1, 1))
    yt = F.conv2d(xp, wt, stride=2)[0]
    yt.backward(torch.tensor(gy))
    y, V = strided_conv(x, w, reflect)
    np.testing.assert_allclose(y, yt.detach().numpy(), atol=1e-11)
    np.testing.assert_allclose(wgrad(V, gy, C), wt.grad.numpy(), atol=1e-10)
    # data gradient: form B on dy with the role-swapped weights (reduction over N); a reflection layer goes through the
    # padded domain and the border fold, a zero-padded one crops
    wsw = w                                                  # wt[cd = n][nout = c]
    if reflect:
        dxp = transposed_conv(gy, wsw, H + 2, W + 2, 1)
        dx = fold_reflect1(dxp)
    else:
        dx = transposed_conv(gy, wsw, H, W, 0)
    np.testing.assert_allclose(dx, xt.grad.numpy(), atol=1e-10)


@pytest.mark.parametrize("Ci,Co,H,W", [(2, 3, 4, 13), (3, 2, 8, 3), (1, 1, 1, 2), (2, 2, 5, 5)])
def test_conv_transpose_all_three_passes(Ci, Co, H, W):
    rng = np.random.default_rng(H * 100 + W)
    d, w = rng.standard_normal((Ci, H, W)), rng.standard_normal((Ci, Co, 4, 4))        # torch ConvTranspose2d weight [Cin,Cout,4,4]
    gz = rng.standard_normal((Co, 2 * H, 2 * W))
    dt, wt = torch.tensor(d, requires_grad=True), torch.tensor(w, requires_grad=True)
    zt = F.conv_transpose2d(dt[None], wt, stride=2, padding=1)[0]
    zt.backward(torch.tensor(gz))
    z = transposed_conv(d, w, 2 * H, 2 * W, 0)
    np.testing.assert_allclose(z, zt.detach().numpy(), atol=1e-11)
    # data gradient = a zero-padded strided conv of dz with the role-swapped weights (conv-form n = Cin_T, c = Cout_T);
    # the weight gradient reduces the SAME transform of dz against the lifted tiles of d
    dd, V = strided_conv(gz, w, False)
    np.testing.assert_allclose(dd, dt.grad.numpy(), atol=1e-10)
    np.testing.assert_allclose(wgrad(V, d, Co), wt.grad.numpy(), atol=1e-10)


def test_fp32_error_stays_near_the_direct_sum():
    rng = np.random.default_rng(0)
    C, H, W = 256, 12, 24
    x = rng.standard_normal((C, H, W)).astype(np.float32)
    w = (rng.standard_normal((C, C, 4, 4)) / np.sqrt(C * 16)).astype(np.float32)
    pad = lambda t: F.pad(t[None], (1, 1, 1, 1), mode="reflect")
    ref = F.conv2d(pad(torch.tensor(x, dtype=torch.float64)), torch.tensor(w, dtype=torch.float64), stride=2)[0].numpy()
    direct = F.conv2d(pad(torch.tensor(x)), torch.tensor(w), stride=2)[0].numpy()
    y, _ = strided_conv(x, w, True, dtype=np.float32)
    scale = np.abs(ref).max()
    e_w = np.sqrt(((y - ref) ** 2).mean()) / scale
    e_d = np.sqrt(((direct - ref) ** 2).mean()) / scale
    print("rms error / max: winograd F(3x3,2x2) %.3e, direct fp32 %.3e" % (e_w, e_d))
    assert e_w < 3e-7 and e_w < 4 * e_d, (e_w, e_d)
