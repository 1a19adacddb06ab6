"""DSR-Splines forward / backward as libsrhip launches (dsr_splines.hip).

Reference: dlib/models/network_dsr_splines.py:283-413 -- bicubic interpolation of the LR input to the HR size (clamped to
[0, 1]); every spline net over the whole image, each result multiplied by the spline's grey-level mask, the sum (+ the
interpolated input under use_global_residual).  With one channel the masks partition the grey levels: one spline
("expert") owns a pixel, and behind the first in_ksz x in_ksz conv every layer is 1x1.  The engine therefore sorts the
pixels by expert on the device (srhip_dsr_splines_order) and runs each pixel's own expert once (srhip_dsr_splines_fwd /
_bwd): 1 / n_splines of the reference's arithmetic and no per-layer feature map.  The interpolation stays on stock
PyTorch-ROCm (F.interpolate, as the reference) and takes no gradient.

Every expert's parameters are contiguous and identically laid out in named_parameters() order, so TrainStep's flat
parameter and gradient buffers already ARE the kernels' [n_splines, P] tables (tensors padded to four floats): they are
used in place when the views line up (data_ptr check); otherwise one launch packs the tensors into a table of the
engine's own (module path) and one unpacks the gradients."""
import torch

from . import ops
from .engine import Engine


class DsrSplinesEngine(Engine):
    need_dx_refusal = "DSR-Splines (libsrhip): no gradient through the bicubic interpolation of the input"

    def __init__(self, net):
        super().__init__(net)
        self.n = net.n_splines
        self.ksz = net.in_ksz
        self.nh = len(net.h_layers)
        self.local = bool(net.use_local_residual)
        self.glob = bool(net.use_global_residual)
        self.P = ops.dsr_splines_table_floats(self.ksz, self.nh, self.local)
        self.names = [k for k, _ in net.named_parameters()]
        self.T = len(self.names) // self.n
        self.lut = None
        self._ptrs = {}
        self.table = self._zeroed = None

    def bucket_prefixes(self):
        """At most 3.8 M parameters, all written by one launch: one gradient bucket."""
        return [["splines."]]

    # ---- parameter / gradient tables
    def _offsets(self, tensors):
        """Element offsets of one expert's tensors in the table layout (each padded to four floats)."""
        offs, off = [], 0
        for t in tensors[:self.T]:
            offs.append(off)
            off += (t.numel() + 3) // 4 * 4
        assert off == self.P, f"DSR-Splines: the module's tensors give {off} floats per expert, the library {self.P}"
        return offs

    def _in_place(self, tensors):
        """[n, P] view over the tensors' storage if they already lie in the table layout, else None."""
        offs = self._offsets(tensors)
        base = tensors[0].data_ptr()
        for k in range(self.n):
            for t in range(self.T):
                if tensors[k * self.T + t].data_ptr() != base + 4 * (k * self.P + offs[t]):
                    return None
        t0 = tensors[0]
        if t0.untyped_storage().nbytes() < 4 * (t0.storage_offset() + self.n * self.P):
            return None
        return t0.as_strided((self.n, self.P), (self.P, 1))

    def _ptr_table(self, key, tensors):
        sig = tuple(t.data_ptr() for t in tensors)
        hit = self._ptrs.get(key)
        if hit is None or hit[0] != sig:
            assert all(t.is_contiguous() and t.dtype == torch.float32 for t in tensors)
            hit = (sig, torch.tensor(sig, dtype=torch.int64).to(tensors[0].device))
            self._ptrs[key] = hit
        return hit[1]

    def prepare(self):
        params = [p.data for _, p in self.net.named_parameters()]
        dev = params[0].device
        if self.lut is None or self.lut.device != dev:
            self.lut = ops.dsr_splines_level_table(self.n, self.net.color_min, self.net.color_max).to(dev)
        tab = self._in_place(params)
        if tab is None:
            tab = self.derived.get("table", self.n, self.P, device=dev)
            if self._zeroed is not tab:                       # the padding floats stay zero
                tab.zero_()
                self._zeroed = tab
            ops.dsr_splines_pack(self._ptr_table("w", params), tab, self.n, self.ksz, self.nh, self.local, to_table=True)
        self.table = tab
        self.prepared = True

    # ---- forward / backward
    def forward(self, x, dp=None, save=True):
        """x [B,h,w] (LR) -> [B,1,s*h,s*w]."""
        return self.forward_interp(self.interpolate(x[:, None]), save=save)

    def forward_interp(self, xi, save=True):
        """xi [B,H,W]: the clamped interpolated image."""
        self.ensure_prepared()
        B, H, W = xi.shape
        pad = (self.ksz - 1) // 2
        if H <= pad or W <= pad:
            raise ValueError(f"DSR-Splines: in_ksz {self.ksz} reflect-pads by {pad}; the interpolated image {H} x {W} needs "
                             f"both sides above that")
        dev = xi.device
        tag = "t" if save else "e"
        N = B * H * W
        ids = self.bufs.get(f"{tag}.ids", B, H, W, device=dev, dtype=torch.uint8)
        order = self.bufs.get(f"{tag}.order", N, device=dev, dtype=torch.int32)
        meta = self.bufs.get(f"{tag}.meta", ops.dsr_splines_meta_ints(N, self.n), device=dev, dtype=torch.int32)
        ops.dsr_splines_order(xi, self.lut, self.n, ids, order, meta)
        y = self.bufs.get("t.y", B, H, W, device=dev) if save else torch.empty(B, H, W, device=dev)
        ops.dsr_splines_fwd(xi, self.table, order, meta, y, self.n, self.ksz, self.nh, self.local, self.glob)
        if save:
            self.saved = dict(xi=xi, order=order, meta=meta, ids=ids)
        self.last_ids = ids
        return y.view(B, 1, H, W)

    def backward(self, dy, grads, need_dx=False, on_layer_done=None, grads_zeroed=False):
        sv = self.saved_for_backward(need_dx)
        xi = sv["xi"]
        gl = [grads[k] for k in self.names]
        gt = self._in_place(gl)
        tmp = gt is None
        if tmp:
            gt = self.derived.get("gtable", self.n, self.P, device=xi.device)
        ops.dsr_splines_bwd(xi, dy.reshape(xi.shape).contiguous(), self.table, sv["order"], sv["meta"], gt, self.n, self.ksz,
                            self.nh, self.local, self.glob)
        if tmp:
            ops.dsr_splines_pack(self._ptr_table("g", gl), gt, self.n, self.ksz, self.nh, self.local, to_table=False)
        return None
