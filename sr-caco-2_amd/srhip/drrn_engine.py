"""DRRN forward / backward as a fixed sequence of libsrhip launches (second of the plain CNNs).

Reference: dlib/models/network_drrn.py:22-126.  bicubic interpolation of the LR input (clamped); conv1 =
ReLU + conv 1->128; a RecursiveBlock that applies ONE residual unit (ReLU, conv, ReLU, conv; shared weights)
num_residual_units times, each time adding the block input; conv2 = ReLU + conv 128->1; + the interpolated
input.  No biases.  Two details of the reference carry over: its ReLUs are in place, so the first ReLU of the
first unit rectifies the block input itself -- the identity that every unit adds is relu(conv1 output), and
the ReLU in front of conv1 acts on an input that is already in [0, 1]:

    x0 = relu(conv1(xi));  r_0 = x0;  a_k = relu(conv_a(r_k));  r_{k+1} = relu(conv_b(a_k) + x0);
    y  = conv2(r_U) + xi

Launches: the 1-channel edge conv with a fused ReLU, 2U split-operand implicit-GEMM convs (epilogues: ReLU /
residual + ReLU, srhip_conv3x3_nhwc_split_ex epi 8), the 128->1 edge conv.  The weight gradients of the
shared convs are summed over the U applications.
"""
import torch

from . import ops
from .engine import Engine

CH = 128


class DRRNEngine(Engine):
    need_dx_refusal = "DRRN (libsrhip): no gradient through the bicubic interpolation of the input"

    def __init__(self, net):
        super().__init__(net)
        self.U = net.trunk.num_residual_unit
        self.ws = ops.WeightSet()
        self.ws.use_bx3 = ops.bx3_nt_for(CH)
        self.saved_h16 = None           # what forward_h16(save=True) kept for backward_h16

    def bucket_prefixes(self):
        """0.30 M parameters: one gradient bucket."""
        return [["conv1.", "trunk.", "conv2."]]

    def _convs(self):
        ru = self.net.trunk.residual_unit
        return [("wa", ru[1]), ("wb", ru[3])]

    def prepare(self):
        self.prepare_conv_packs((name, conv.weight.data, False) for name, conv in self._convs())

    def amp_train_ok(self):
        """Whether this configuration trains under --amp on fp16 storage (forward_h16(save=True) + backward_h16): the fp16x2
        packs of both shared convs in both directions."""
        self.ensure_prepared()
        return self.ws.use_bx3 and all(self.ws[n + s].fmt == 1 for n, _ in self._convs() for s in (".wp", ".wpt"))

    def _amp_train_refusal(self):
        return (f"DRRN under --amp training runs on fp16 storage only with the fp16x2 packs of both shared convs in both "
                f"directions; this net: fp16x2 packs {self.ws.use_bx3 and self.ws['wa.wp'].fmt == 1} (SRHIP_MM / "
                f"SRHIP_F16X2_CONV switch them off)")

    def forward_h16(self, x, save=False):
        """fp16 storage (conv_h16.hip): the same launches with float16 feature maps, one fp16 product.  save=False: --amp
        evaluation ("h." buffers, two rotating unit outputs).  save=True: the --amp training forward (autocast's fp16 maps,
        model_plain.py:322-327): x0 and every unit's a_k, r_{k+1} are kept in "a." buffers of their own -- an evaluation
        forward in between overwrites none of them."""
        self.ensure_prepared()
        if save and not self.amp_train_ok():
            raise NotImplementedError(self._amp_train_refusal())
        net, U = self.net, self.U
        xi = self.interpolate(x[:, None])
        B, H, W = xi.shape
        tag = "a." if save else "h."

        def buf(name):
            return self.bufs.get(tag + name, B, H, W, CH, device=x.device, dtype=torch.float16)
        x0 = ops.conv3x3_cin1_h16(xi, net.conv1[1].weight.data, None, CH, out=buf("x0"), relu=True)
        r = x0
        rs, as_ = [], []
        for k in range(U):
            a = ops.conv3x3_h16(r, self.ws["wa.wp"], None, CH, out=buf(f"a{k}" if save else "a"), epi=1)
            rs.append(r)
            as_.append(a)
            r = ops.conv3x3_h16(a, self.ws["wb.wp"], None, CH, out=buf(f"r{k + 1 if save else k % 2}"), epi=8, R=x0)
        # (training: the f32 output in the f32 step's own buffer, which ModelPlain.E reads)
        y = ops.conv3x3_cout1_h16(r, net.conv2[1].weight.data, None, add=xi,
                                  out=self.bufs.get("t.y", B, H, W, device=x.device) if save else None)
        if save:
            self.saved_h16 = dict(xi=xi, x0=x0, rs=rs, as_=as_, r_last=r, B=B, H=H, W=W)
        return y.view(B, 1, H, W)

    def forward(self, x, dp=None, save=True):
        """x [B,H,W] (LR) -> [B,1,s*H,s*W]."""
        self.ensure_prepared()
        if not save and ops.h16_eval() and self.ws.use_bx3 and self.ws["wa.wp"].fmt == 1:
            self.last_eval_path = "fp16 storage"
            return self.forward_h16(x)
        net, U = self.net, self.U
        xi = self.interpolate(x[:, None])
        B, H, W = xi.shape
        dev = x.device
        buf = self.bufs.tagged("t." if save else "e.", dev)
        x0 = buf("x0", B, H, W, CH)
        ops.conv3x3_cin1_fwd(xi, net.conv1[1].weight.data, None, CH, out=x0, relu=True)
        r = x0
        rs, as_ = [], []
        for k in range(U):
            a = buf(f"a{k if save else 0}", B, H, W, CH)
            ops.conv3x3(r, self.ws["wa.wp"], None, CH, out=a, epi=1)
            rn = buf(f"r{k + 1 if save else 1 + k % 2}", B, H, W, CH)
            if self.ws.use_bx3:                              # r_{k+1} = relu(conv_b(a_k) + x0): residual + ReLU as the epilogue
                ops.conv3x3(a, self.ws["wb.wp"], None, CH, out=rn, epi=8, R=x0)
            else:
                ops.conv3x3(a, self.ws["wb.wp"], None, CH, out=rn, epi=2, R=x0)
                ops.relu_mask(rn, rn)
            if save:
                rs.append(r)
                as_.append(a)
            r = rn
        y = torch.empty(B, H, W, device=dev) if not save else buf("y", B, H, W)
        ops.conv3x3_cout1_fwd(r, net.conv2[1].weight.data, None, out=y)
        ops.axpby(y, xi, 1.0, 1.0)
        if save:
            self.saved = dict(xi=xi, x0=x0, rs=rs, as_=as_, r_last=r, B=B, H=H, W=W)
        return y.view(B, 1, H, W)

    def backward(self, dy, grads, need_dx=False, on_layer_done=None, grads_zeroed=False):
        sv = self.saved_for_backward(need_dx)
        net, U = self.net, self.U
        B, H, W = sv["B"], sv["H"], sv["W"]
        buf = self.bufs.tagged("g.", dy.device)
        dy = dy.reshape(B, H, W).contiguous()
        ops.conv3x3_cin1_wgrad(dy, sv["r_last"], grads["conv2.1.weight"], None, flip=True)
        gu, ga, gx0 = buf("gu", B, H, W, CH), buf("ga", B, H, W, CH), buf("gx0", B, H, W, CH)
        ops.conv3x3_cin1_fwd(dy, net.conv2[1].weight.data, None, CH, out=gu, flip=True)
        ops.relu_mask(gu, sv["r_last"])                      # through r_U = relu(u_U)
        dWa, dWb = grads["trunk.residual_unit.1.weight"], grads["trunk.residual_unit.3.weight"]
        tWa, tWb = buf("tWa", CH, CH, 3, 3), buf("tWb", CH, CH, 3, 3)
        gx0.zero_()
        for k in reversed(range(U)):                         # gu = d / d u_{k+1}, u_{k+1} = conv_b(a_k) + x0
            ops.axpby(gx0, gu, 1.0, 1.0)                     # the identity path of every unit
            first = k == U - 1
            ops.conv3x3_wgrad(gu, sv["as_"][k], dWb if first else tWb, None)
            ops.conv3x3(gu, self.ws["wb.wpt"], None, CH, out=ga, epi=4, R=sv["as_"][k])     # * (a_k > 0)
            ops.conv3x3_wgrad(ga, sv["rs"][k], dWa if first else tWa, None)
            if not first:                                    # shared weights: sum over the applications
                ops.axpby(dWb, tWb, 1.0, 1.0)
                ops.axpby(dWa, tWa, 1.0, 1.0)
            # d / d r_k, masked by r_k > 0: for k >= 1 that is the unit's ReLU (-> d / d u_k); for k = 0
            # it is the in-place ReLU that made x0 out of conv1's output
            ops.conv3x3(ga, self.ws["wa.wpt"], None, CH, out=gu, epi=4, R=sv["rs"][k])
        ops.relu_mask(gx0, sv["x0"])
        ops.axpby(gu, gx0, 1.0, 1.0)                         # d / d conv1 output
        ops.conv3x3_cin1_wgrad(sv["xi"], gu, grads["conv1.1.weight"], None)
        # single bucket = the last one: TrainStep's reducer sends it after backward (announcing it
        # here too reduced it twice -- the sum instead of the mean -- before the reducer tracked
        # which buckets were done)
        return None

    def backward_h16(self, dy, grads, need_dx=False, on_layer_done=None, grads_zeroed=False):
        """backward() on fp16 storage (the reference's backward under autocast: fp16 activation gradients, fp16 products, f32
        accumulation; model_plain.py:348): dy f32 (the loss gradient, already times the loss scale) -> grads (f32).

        Per unit k = U-1 .. 0, with gu = d / d u_{k+1} (fp16):
          ga    = (a_k > 0) * conv_b^T(gu)                       conv3x3_h16 epi 9
          dW_b += gu (x) a_k,  dW_a += ga (x) r_k                one shared-weight weight-gradient launch (unit 0 of the
                                                                 backward, k = U-1, overwrites; the others add, in order)
          gu'   = (r_k > 0) * conv_a^T(ga),  G += gu'            k >= 1: the identity gradient into x0 rides in the epilogue
          g_c1  = (x0 > 0) * (conv_a^T(ga) + G)                  k = 0: r_0 IS x0; the sum ends there
        G (f32) starts as gu_U from the tail.  The shared weights' gradient is summed in f32 across the units (autograd sums
        the fp16 per-application gradients of autocast's cached fp16 weight copy in fp16)."""
        sv = self.saved_h16
        assert sv is not None, "backward_h16() without a saved forward_h16(save=True)"
        assert not need_dx, self.need_dx_refusal
        net, U = self.net, self.U
        B, H, W = sv["B"], sv["H"], sv["W"]
        dev = dy.device

        def buf(name, dtype=torch.float16):
            return self.bufs.get("ag." + name, B, H, W, CH, device=dev, dtype=dtype)

        dy = dy.reshape(B, H, W).contiguous()
        ops.conv3x3_cin1_wgrad_h16(dy, sv["r_last"], grads["conv2.1.weight"], None, flip=True)
        gus = [buf("gu0"), buf("gu1")]
        ga, G = buf("ga"), buf("gx0", torch.float32)
        gu = ops.conv3x3_cin1_h16_flip_mask(dy, net.conv2[1].weight.data, sv["r_last"], gus[U % 2], G)
        dWa, dWb = grads["trunk.residual_unit.1.weight"], grads["trunk.residual_unit.3.weight"]
        for k in reversed(range(U)):
            ops.conv3x3_h16(gu, self.ws["wb.wpt"], None, CH, out=ga, epi=9, R=sv["as_"][k], alpha=1.0)
            ops.conv3x3_wgrad_shared_h16([(gu, sv["as_"][k], dWb, None), (ga, sv["rs"][k], dWa, None)],
                                         accumulate=k < U - 1)
            gu = ops.conv3x3_dgrad_relu_acc_h16(ga, self.ws["wa.wpt"], sv["rs"][k], gus[k % 2], G, mode=0 if k else 1)
        ops.conv3x3_cin1_wgrad_h16(sv["xi"], gu, grads["conv1.1.weight"], None)
        # single bucket = the last one: TrainStep's reducer sends it after backward
        return None
