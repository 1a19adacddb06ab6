"""What every engine shares: the named buffer set (``Bufs``), the interpolation in front of the refining nets and the
base class ``Engine`` -- the one statement of what the training loop, the mirrors and the tools read from an engine."""
import torch
import torch.nn.functional as F

from . import ops


class Bufs:
    """Persistent activation / gradient buffers keyed by name (no allocation in
    the steady-state step; also what makes the step graph-capturable)."""

    def __init__(self):
        self.d = {}
        self.pool = None        # the training buffers of a tape graph by shape (tape.py: the first recording Tape makes it)

    def get(self, key, *shape, device="cuda", dtype=torch.float32):
        t = self.d.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            if t is not None:
                ops.note_realloc()      # a replaced buffer is freed: captured graphs holding its address must be re-made
            t = torch.empty(shape, device=device, dtype=dtype)
            self.d[key] = t
        return t

    def tagged(self, prefix, device, dtype=torch.float32):
        """``buf(name, *shape)``: get() under the key ``prefix + name``"""
        def buf(name, *shape):
            return self.get(prefix + name, *shape, device=device, dtype=dtype)
        return buf

    def clear(self):
        if self.d:
            ops.note_realloc()
        self.d.clear()


def bicubic_clamped(x, scale):
    """[B,1,h,w] -> [B,s*h,s*w]: the bicubic interpolation (align_corners False), clamped to [0, 1], in front of the nets
    that refine an interpolated input (VDSR, DRRN, MemNet, DSR-Splines) -- stock PyTorch-ROCm, as in the reference."""
    out = F.interpolate(x, size=(scale * x.shape[2], scale * x.shape[3]), mode='bicubic', align_corners=False)
    return torch.clamp(out, min=0.0, max=1.0)[:, 0].contiguous()


class Engine:
    """Base of the seventeen engines: one net's forward and backward as libsrhip launches.

    What train.py, model_plain.py, predict.py, bench.py and the mirrors (dlib/models/engine_net.py) read from an engine:
      ``forward(x, dp=None, save=...)`` -> the output image; ``save=True`` keeps what ``backward(dy, grads, need_dx=False,
        on_layer_done=None, grads_zeroed=False)`` reads in ``saved`` (None until then) and writes the "t." buffers,
        ``save=False`` the "e." ones; ``backward`` fills ``grads`` (name -> tensor) and returns dx or None;
      ``invalidate()``: the parameters changed, the derived weights are stale (``prepared`` False; the next forward runs
        ``prepare()``);
      ``bucket_prefixes()``: the gradient buckets of a data-parallel step as lists of parameter-name prefixes, in the order
        backward completes them (``on_layer_done(i)`` announces every bucket but the last);
      ``train_graph_default``: ModelPlain replays the training step from a hipGraph (TrainStep.step_graph) unless told otherwise;
      ``bufs`` (activations and gradients by name), ``derived`` (weight copies by name), ``net``.
    Present only on the engines that have them -- their presence is the signal, so this class defines none:
      ``forward_h16`` / ``backward_h16`` (fp16 storage: --amp evaluation / training), ``amp_train_ok`` and
      ``_amp_train_refusal`` (--amp training), ``intermediate_outs`` (the multi-scale losses), ``taps`` (tests),
      ``layer0_bucket_groups``, and ``last_eval_path``: an instance attribute from the first fp16-storage evaluation
      forward on, never cleared.
    An engine that picks its matmul operands by a rule of its own keeps its ``ws = ops.WeightSet()`` beside that rule."""
    train_graph_default = False
    need_dx_refusal = None          # the text backward() refuses need_dx with (None: the engine returns dx)
    need_dx_error = AssertionError

    def __init__(self, net):
        self.net = net
        self.bufs = Bufs()
        self.derived = Bufs()
        self.prepared = False
        self.saved = None
        self._prep = self._prep_sig = None

    def invalidate(self):
        self.prepared = False

    def bucket_prefixes(self):
        return [[""]]           # one gradient bucket: every parameter

    def ensure_prepared(self):
        if not self.prepared:
            self.prepare()

    def prep_table(self, fill, before_run=None):
        """The cached job table of the per-step weight preparation: ``fill(tb)`` lays the jobs out on a fresh ops.PrepTable
        when there is none yet or a parameter of the net moved (data_ptr); otherwise -- and then too -- one run().
        before_run(): what has to be written behind a rebuild's own launches and in front of the run (SRCNN's padded copies)."""
        sig = tuple(p.data_ptr() for p in self.net.parameters())
        if self._prep is None or sig != self._prep_sig:
            tb = ops.PrepTable()
            fill(tb)
            self._prep, self._prep_sig = tb.build(next(self.net.parameters()).device), sig
        if before_run is not None:
            before_run()
        self._prep.run()

    def prepare_conv_packs(self, convs):
        """prepare() of an engine whose derived weights are the packs of its 3x3 convs, ``convs`` an iterable of (name, weight
        [Co,Ci,3,3], ps2) -- read only when the packs are laid out, so a generator costs a steady-state step nothing.  Planes:
        the cached job table; exact-f32 kernels: the packs in ``derived``."""
        ws = self.ws
        if ws.use_bx3:
            def fill(tb):
                for name, w, ps2 in convs:
                    tb.conv_pair(name, w, ws, ps2=ps2)
            self.prep_table(fill)
        else:
            for name, w, _ in convs:
                ws.pack_conv(name, w, self.derived)
        self.prepared = True

    def interpolate(self, x):
        return bicubic_clamped(x, self.net.upscale)

    def saved_for_backward(self, need_dx=False):
        """what opens every backward(): the saved forward, or the engine's refusal of the input gradient"""
        assert self.saved is not None, "backward() without a saved forward"
        if need_dx and self.need_dx_refusal is not None:
            raise self.need_dx_error(self.need_dx_refusal)
        return self.saved
