"""DSR-Splines restated in the one-expert-per-pixel form, in plain torch on the CPU (float32 or float64, autograd).

Written from the semantics, not from the reference's code: the interpolated image is clamp(bicubic(x), 0, 1); a pixel's
expert is the bin of np.array_split(range(256), n) that holds uint8(float32(v) * 255.0f); the expert is a small net on the
pixel's reflect-padded in_ksz x in_ksz neighbourhood -- layer 0 a conv of that size, every later layer 1x1, widths
``hidden`` then 1; a layer is act(conv(x)), or act(relu(conv(x)) + match_sz(x)) under the local residual (match_sz a biased 1x1
conv where the widths differ, the identity where they agree); act is ReLU, tanh for the last layer under the global residual,
which also adds the interpolated image to the output."""
import numpy as np
import torch
import torch.nn.functional as F

HIDDEN = {f"snet_type{i + 1}": [32] * i + [16] for i in range(8)}


def level_table(n):
    """256 grey levels -> expert: the bins of np.array_split(range(256), n)."""
    lut = np.empty(256, dtype=np.int64)
    for k, s in enumerate(np.array_split(np.arange(256), n)):
        lut[s] = k
    return lut


def expert_ids(x_interp, n):
    """x_interp: float32 array / tensor -> int64 array of the same shape.  The product is taken in float32 and truncated."""
    v = np.asarray(x_interp, dtype=np.float32)
    u = np.clip((v * np.float32(255.0)).astype(np.uint8).astype(np.float32), 0, 255).astype(np.int64)
    return level_table(n)[u]


def interpolate(x, scale):
    out = F.interpolate(x, size=(scale * x.shape[2], scale * x.shape[3]), mode='bicubic', align_corners=False)
    return torch.clamp(out, min=0.0, max=1.0)


def layout(in_ksz, hidden, n, local):
    """(key, shape) of the state_dict, in the module's order."""
    widths = [1] + list(hidden) + [1]
    out = []
    for k in range(n):
        for i in range(len(widths) - 1):
            ci, co, ks = widths[i], widths[i + 1], in_ksz if i == 0 else 1
            pre = f"splines.{k}.model.{i}."
            out += [(pre + "conv.weight", (co, ci, ks, ks)), (pre + "conv.bias", (co,))]
            if local and ci != co:
                out += [(pre + "match_sz.weight", (co, ci, 1, 1)), (pre + "match_sz.bias", (co,))]
    return out


def forward(sd, xi, ids, hidden, in_ksz, local, glob):
    """sd: state dict (tensors of xi's dtype, leaves for autograd), xi [B,1,H,W] the interpolated image, ids [B,H,W] int64
    (array or tensor) -> y [B,1,H,W]."""
    B, _, H, W = xi.shape
    pad = (in_ksz - 1) // 2
    xp = F.pad(xi, (pad, pad, pad, pad), mode='reflect') if pad else xi
    patches = F.unfold(xp, in_ksz).transpose(1, 2).reshape(B * H * W, in_ksz * in_ksz)
    centre = xi.reshape(-1, 1)
    flat = torch.as_tensor(np.asarray(ids)).reshape(-1)
    nl = len(hidden) + 1
    idxs, vals = [], []
    for e in torch.unique(flat).tolist():
        idx = (flat == e).nonzero()[:, 0]
        a, skip = patches[idx], centre[idx]
        for i in range(nl):
            pre = f"splines.{e}.model.{i}."
            w = sd[pre + "conv.weight"]
            s = a @ w.reshape(w.shape[0], -1).t() + sd[pre + "conv.bias"]
            if local:
                if pre + "match_sz.weight" in sd:
                    mw = sd[pre + "match_sz.weight"]
                    skip = skip @ mw.reshape(mw.shape[0], -1).t() + sd[pre + "match_sz.bias"]
                s = torch.relu(s) + skip
            a = torch.tanh(s) if (glob and i == nl - 1) else torch.relu(s)
            skip = a
        idxs.append(idx)
        vals.append(a[:, 0])
    y = torch.zeros(B * H * W, dtype=xi.dtype).index_add(0, torch.cat(idxs), torch.cat(vals)).view(B, 1, H, W)
    return y + xi if glob else y


def loss_and_grads(sd, xi, ids, tgt, hidden, in_ksz, local, glob, dtype, dy=None):
    """L1 (mean) loss against tgt -- or, with dy, the loss sum(y * dy), whose output gradient is dy itself -- and the
    gradient of every parameter, in `dtype`."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    y = forward(leaves, xi.to(dtype), ids, hidden, in_ksz, local, glob)
    loss = (y - tgt.to(dtype)).abs().mean() if dy is None else (y * dy.to(dtype)).sum()
    loss.backward()
    return y.detach(), loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
