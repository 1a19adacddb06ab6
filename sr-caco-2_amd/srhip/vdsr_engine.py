"""VDSR forward / backward as a fixed sequence of libsrhip launches (the plain CNNs reuse the
3x3-conv kernels).

Reference: dlib/models/network_vdsr.py:24-126 -- bicubic interpolation of the LR input to the HR size
(clamped to [0, 1]); conv1 1->64 + ReLU; 18 x (conv 64->64 + ReLU); conv2 64->1; + the interpolated input.
No biases.  The interpolation stays on stock PyTorch-ROCm (F.interpolate, as the reference); every conv is a
libsrhip kernel: the 1-channel edge convs of small.hip, the bf16x3 implicit-GEMM conv with the ReLU as its
epilogue, the ReLU mask of the backward as the data-gradient conv's epilogue (epi 4).  NHWC throughout.
"""
import torch

from . import ops
from .engine import Engine

CH = 64


class VDSREngine(Engine):
    need_dx_refusal = "VDSR (libsrhip): no gradient through the bicubic interpolation of the input"

    def __init__(self, net):
        super().__init__(net)
        self.nt = len(net.trunk)
        self.ws = ops.WeightSet()
        self.ws.use_bx3 = ops.bx3_nt_for(CH)

    def bucket_prefixes(self):
        """0.67 M parameters: one gradient bucket."""
        return [["conv1.", "trunk.", "conv2."]]

    def prepare(self):
        self.prepare_conv_packs((f"t{k}", self.net.trunk[k].conv.weight.data, False) for k in range(self.nt))

    def forward_h16(self, x):
        """--amp evaluation on fp16 storage (conv_h16.hip): the same launches with float16 feature maps, one fp16 product."""
        net = self.net
        xi = self.interpolate(x[:, None])
        B, H, W = xi.shape
        a = self.bufs.get("h.a0", B, H, W, CH, device=x.device, dtype=torch.float16)
        ops.conv3x3_cin1_h16(xi, net.conv1[0].weight.data, None, CH, out=a, relu=True)
        for k in range(self.nt):
            an = self.bufs.get(f"h.a{1 + k % 2}", B, H, W, CH, device=x.device, dtype=torch.float16)
            ops.conv3x3_h16(a, self.ws[f"t{k}.wp"], None, CH, out=an, epi=1)
            a = an
        y = ops.conv3x3_cout1_h16(a, net.conv2.weight.data, None, add=xi)       # + the interpolated input
        return y.view(B, 1, H, W)

    def forward(self, x, dp=None, save=True):
        """x [B,H,W] (LR) -> [B,1,s*H,s*W]."""
        self.ensure_prepared()
        if not save and ops.h16_eval() and self.ws.use_bx3 and self.ws["t0.wp"].fmt == 1:
            self.last_eval_path = "fp16 storage"
            return self.forward_h16(x)
        net = self.net
        xi = self.interpolate(x[:, None])
        B, H, W = xi.shape
        dev = x.device
        buf = self.bufs.tagged("t." if save else "e.", dev)
        a = buf("a0", B, H, W, CH)
        ops.conv3x3_cin1_fwd(xi, net.conv1[0].weight.data, None, CH, out=a, relu=True)
        acts = [a]
        for k in range(self.nt):
            an = buf(f"a{k + 1 if save else 1 + k % 2}", B, H, W, CH)
            ops.conv3x3(a, self.ws[f"t{k}.wp"], None, CH, out=an, epi=1)
            if save:
                acts.append(an)
            a = an
        y = torch.empty(B, H, W, device=dev) if not save else buf("y", B, H, W)
        ops.conv3x3_cout1_fwd(a, net.conv2.weight.data, None, out=y)
        ops.axpby(y, xi, 1.0, 1.0)                       # + the interpolated input (global residual)
        if save:
            self.saved = dict(xi=xi, acts=acts, B=B, H=H, W=W)
        return y.view(B, 1, H, W)

    def backward(self, dy, grads, need_dx=False, on_layer_done=None, grads_zeroed=False):
        sv = self.saved_for_backward(need_dx)
        net = self.net
        B, H, W = sv["B"], sv["H"], sv["W"]
        dev = dy.device
        acts = sv["acts"]
        buf = self.bufs.tagged("g.", dev)
        dy = dy.reshape(B, H, W).contiguous()
        # conv2 (64 -> 1): weight gradient = the 1-channel kernel with x / dy swapped and flipped taps,
        # data gradient = the 1-channel forward kernel with flipped taps; then the last ReLU's mask
        ops.conv3x3_cin1_wgrad(dy, acts[-1], grads["conv2.weight"], None, flip=True)
        ga, gb = buf("ga", B, H, W, CH), buf("gb", B, H, W, CH)
        g = ga
        ops.conv3x3_cin1_fwd(dy, net.conv2.weight.data, None, CH, out=g, flip=True)
        ops.relu_mask(g, acts[-1])
        for k in reversed(range(self.nt)):               # a_{k+1} = relu(conv_k(a_k)); g = d/d(conv_k output)
            ops.conv3x3_wgrad(g, acts[k], grads[f"trunk.{k}.conv.weight"], None)
            other = gb if g is ga else ga
            ops.conv3x3(g, self.ws[f"t{k}.wpt"], None, CH, out=other, epi=4, R=acts[k])     # * (a_k > 0)
            g = other
        ops.conv3x3_cin1_wgrad(sv["xi"], g, grads["conv1.0.weight"], None)
        # single bucket = the last one: TrainStep's reducer sends it after backward (announcing it
        # here too reduced it twice -- the sum instead of the mean -- before the reducer tracked
        # which buckets were done)
        return None
