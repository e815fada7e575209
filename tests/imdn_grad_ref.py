"""Gradients of one IMDN_RTC net with IMDN2.predict's clamp and affine, by torch autograd through
imdn_ref64.torch_imdn_rtc in any dtype and on any device, and the screened batches of test_gpu_imdn_train_tiles.py (a
helper for test_imdn_grad_cpu.py, test_imdn_hazard_cpu.py and the test_gpu_imdn_train*.py files, not a test).  The clamp is restated on its own: the cotangent of the raw output y is G * factor * [-1 <= y <= 1] with the
factor 127 (post 1) or 1/2 (post 2), torch.clamp's derivative, so the checker does not lean on autograd for the mask."""
import numpy as np

import imdn_ref64 as R


def net_keys(sd, prefix):
    return [k for k in sd if k.startswith(prefix)]


def net_grads(torch, sd, prefix, x, G, post, dtype, device="cpu"):
    """sd {key: float32 array}, x and G arrays -> (raw output y, {key: gradient}, grad_x) as float64 numpy arrays: the
    gradients of sum(G * post(net(x))), computed in `dtype` on `device`"""
    keys = net_keys(sd, prefix)
    sdt = {k: torch.tensor(sd[k], dtype=dtype, device=device).requires_grad_() for k in keys}
    xt = torch.tensor(np.asarray(x), dtype=dtype, device=device).requires_grad_()
    y = R.torch_imdn_rtc(sdt, prefix, xt)
    gy = torch.tensor(np.asarray(G), dtype=dtype, device=device)
    if post:
        yd = y.detach()
        gy = gy * (127.0 if post == 1 else 0.5) * ((yd >= -1) & (yd <= 1)).to(dtype)
    y.backward(gy)
    to64 = lambda t: t.detach().double().cpu().numpy()
    return to64(y), {k: to64(sdt[k].grad) for k in keys}, to64(xt.grad)


Z_WIDTH = 1e-5      # about ten times the largest float32-against-float64 difference of these nets (1.35e-6 on the raw output)
Y_WIDTH = 1e-4      # test_gpu_imdn_train.py's distance of every raw output from +-1


def screened_batch(sd, prefix, nf, in_nc, out_nc, B, H, W, post, seed, exempt=()):
    """A batch on which no float32 run can flip a LeakyReLU sign or the clamp mask -> (x [B, in_nc, H, W], G [B, out_nc, H, W],
    kept share).  From default_rng(seed + 1): a pool of 4 B images, uniform on [0, 3) as in test_gpu_imdn_train.py's
    _case, of which the first B with imdn_ref64.hazards' zmin > Z_WIDTH and (post != 0) ymin > Y_WIDTH are kept, then a
    normal G.  The pool size is a condition: fewer than B survivors raise."""
    assert sd[prefix + "model.0.weight"].shape[:2] == (nf, in_nc) and sd[prefix + "model.2.weight"].shape[0] == out_nc
    rng = np.random.default_rng(seed + 1)
    pool = (3 * rng.random((4 * B, in_nc, H, W))).astype(np.float32)
    zmin, ymin = R.hazards(sd, prefix, pool, exempt)
    keep = zmin > Z_WIDTH
    if post:
        keep &= ymin > Y_WIDTH
    if int(keep.sum()) < B:
        raise ValueError("only %d of %d images pass the hazard screen, %d are needed" % (int(keep.sum()), 4 * B, B))
    x = np.ascontiguousarray(pool[keep][:B])
    G = rng.standard_normal((B, out_nc, H, W)).astype(np.float32)
    return x, G, float(keep.mean())


def rel_err(t, t64):
    """max |t - t64| / max |t64|"""
    return float(np.abs(np.asarray(t, np.float64) - t64).max() / max(np.abs(t64).max(), 1e-300))
