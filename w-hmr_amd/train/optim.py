"""FusedAdam: the optimizer step of the training iteration (core/trainer.py:615, ``self.optimizer.step()``) as two HIP launches over a device-resident
table (csrc/adam.hip), capturable in a HIP graph, which also writes the bf16 W / W^T operand copies of the ViT's weights.

Arithmetic: torch's non-amsgrad Adam with L2 weight decay, fp32; state keys and ``state_dict()`` layout are torch's (``step`` a 0-dim fp32 device
tensor as with ``capturable=True``), so checkpoints interchange with ``torch.optim.Adam(capturable=True)`` in both directions.

What lives where:

* step counts, bias corrections, hyper-parameters: device memory.  ``param_groups[i]['lr']`` stays a Python float (the reference's decay loop,
  trainer.py:331-337, multiplies it); an eager ``step()`` pushes changed rows to the device, ``sync_hyperparameters()`` does it between replays
  of a captured step.
* the table (one ``struct whmr_adam_item`` per parameter with a gradient): rebuilt whenever a pointer of a (parameter, gradient, state) triple
  differs from the last upload -- eager steps with ``p.grad = None`` get new gradient tensors every iteration -- and uploaded with a non-blocking
  copy from a pinned staging buffer that is never rewritten (a copy recorded during a capture replays from that host memory).
* ``step()`` never synchronises and never reads device memory on the host.

The library's weight caches are keyed on ``Parameter._version`` (models/*: ``_wcache``, L.WeightOperands); torch's in-place update bumps it, a
raw kernel does not, so ``step()`` calls ``torch.autograd.graph.increment_version`` on every parameter it updated (and ``mark_updated()`` does the
same after a graph replay, where no Python of ``step()`` runs).
"""
import ctypes
import struct

import torch

from .. import _lib as L

_ITEM = struct.Struct('<7Qq6i2d')              # struct whmr_adam_item (include/whmr_hip.h; ctypes mirror: _lib._WhmrAdamItem)
assert _ITEM.size == ctypes.sizeof(L._WhmrAdamItem)
_HYPER = struct.Struct('<3d2f')                 # struct whmr_adam_hyper: betas and lr as doubles (1 - beta, 1 - beta^t and lr / bc1 are formed in double on the device)
assert _HYPER.size == ctypes.sizeof(L._WhmrAdamHyper)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, differentiable=False):
        for name, value in (('amsgrad', amsgrad), ('maximize', maximize), ('differentiable', differentiable)):
            if value:
                raise ValueError('FusedAdam implements plain Adam only: %s is not supported' % name)
        # every key torch.optim.Adam keeps in a group, so that a state_dict() of either loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=True,
                        differentiable=False, fused=None, decoupled_weight_decay=False)
        self._device = None
        self._wo = None                 # attached L.WeightOperands
        self._key = None                # pointers of the last upload
        self._n_items = self._blocks = 0
        self._table = self._hyper = self._hyper_pushed = None
        self._staging = self._hyper_staging = self._spare = None
        self._graph_staging = []        # staging buffers of uploads recorded into a graph: a replay copies from them
        self._updated = []
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    # ------------------------------------------------------------------ validation
    @staticmethod
    def _check_group(group):
        if isinstance(group['lr'], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group['betas']):
            raise ValueError('FusedAdam keeps lr and betas as Python floats (the device rows are pushed by step() / sync_hyperparameters())')
        for name in ('amsgrad', 'maximize', 'differentiable', 'decoupled_weight_decay'):
            if group.get(name):
                raise ValueError('FusedAdam implements plain Adam only: %s is not supported' % name)
        b1, b2 = group['betas']
        if group['lr'] < 0.0 or group['eps'] < 0.0 or group['weight_decay'] < 0.0 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError('invalid Adam hyper-parameters: %r' % {k: group[k] for k in ('lr', 'betas', 'eps', 'weight_decay')})

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        for p in group['params']:
            if p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous():
                raise ValueError('FusedAdam updates dense contiguous fp32 parameters (got %s, strides %s)' % (p.dtype, tuple(p.stride())))
            if not p.is_cuda:
                raise ValueError('FusedAdam updates HIP device tensors only (got a parameter on %s); there is no CPU fallback' % p.device)
            if self._device is None:
                self._device = p.device
            elif p.device != self._device:
                raise ValueError('FusedAdam keeps one device table: all parameters on %s (got %s)' % (self._device, p.device))
        self._key = None

    def load_state_dict(self, state_dict):
        """Accepts what torch.optim.Adam writes, capturable or not (the reference checkpoints a default Adam, trainer.py:362): torch leaves ``step`` of a
        non-capturable checkpoint on the host (or as a Python number in old files) and takes the group's flags from the file; here every ``step``
        becomes a 0-dim fp32 tensor on the parameter's device, exp_avg / exp_avg_sq contiguous fp32 tensors there, and the groups are capturable
        again -- the kernels dereference all three."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
            group['capturable'] = True
            group['foreach'] = group['fused'] = None
            for p in group['params']:
                st = self.state.get(p)
                if not st:
                    continue
                missing = [k for k in ('step', 'exp_avg', 'exp_avg_sq') if k not in st]
                if missing:
                    raise ValueError('FusedAdam.load_state_dict: state of a parameter lacks %s' % missing)
                st['step'] = torch.as_tensor(st['step']).detach().to(dtype=torch.float32, device=p.device).reshape(())
                for k in ('exp_avg', 'exp_avg_sq'):
                    t = st[k]
                    if not isinstance(t, torch.Tensor) or t.shape != p.shape:
                        raise ValueError('FusedAdam.load_state_dict: %s does not have its parameter\'s shape %s' % (k, tuple(p.shape)))
                    st[k] = t.detach().to(dtype=torch.float32, device=p.device).contiguous()
        self._key = None

    # ------------------------------------------------------------------ operands
    @property
    def operands(self):
        return self._wo

    def attach_operands(self, wo):
        """wo: L.WeightOperands.  Its matrices are updated tile by tile from now on and the same pass writes ``wo.copies`` (W and W^T in bf16), so that
        ``wo.refresh()`` has nothing to launch after a step.  Parameters of ``wo`` this optimizer does not hold keep being served by refresh()."""
        wo.refresh()                    # from here on the copies are current whenever wo.versions says so
        self._wo = wo
        self._key = None

    def detach_operands(self):
        self._wo = None
        self._key = None

    @classmethod
    def for_model(cls, model, **kw):
        """The optimizer over ``model.parameters()``; in the bf16 numerics the ViT backbone's operand copies (created here if the first training forward
        has not made them yet) are attached."""
        from ..models.pose_vit import ViT
        from .vit_autograd import _weight_operands
        opt = cls(model.parameters(), **kw)
        vit = next((m for m in model.modules() if isinstance(m, ViT)), None)
        if vit is not None and vit.numerics == 'bf16':
            _weight_operands(vit)
            opt.attach_operands(vit.__dict__['_train_operands'])
        return opt

    # ------------------------------------------------------------------ device rows
    def _rows(self):
        return [(float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay'])) for g in self.param_groups]

    def sync_hyperparameters(self):
        """Push lr / betas / eps / weight_decay of every group to the device rows if they changed (on the current stream, no synchronisation).
        An eager step() does this itself; between two replays of a captured step it is the caller's line after changing ``param_groups``."""
        rows = self._rows()
        if rows == self._hyper_pushed:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdam: hyper-parameters changed inside a graph capture; the recorded copy would reset them at every replay -- '
                               'run a warm-up step (or sync_hyperparameters()) before the capture')
        for g in self.param_groups:
            self._check_group(g)
        with torch.cuda.device(self._device):
            if self._hyper is not None and self._hyper.numel() != len(rows) * _HYPER.size and self._graph_staging:
                raise RuntimeError('FusedAdam: the number of parameter groups changed after a step was captured; the graph holds the old rows -- '
                                   'build a new optimizer and capture again')
            if self._hyper is None or self._hyper.numel() != len(rows) * _HYPER.size:
                self._hyper = torch.zeros(len(rows) * _HYPER.size, dtype=torch.uint8, device=self._device)
            blob = b''.join(_HYPER.pack(b1, b2, lr, eps, wd) for lr, b1, b2, eps, wd in rows)
            self._hyper_staging = torch.frombuffer(bytearray(blob), dtype=torch.uint8).pin_memory()     # a fresh buffer per push: the copy in flight
                                                                                                         # reads the previous one
            self._hyper.copy_(self._hyper_staging, non_blocking=True)
        self._hyper_pushed = rows

    def _capacity(self):
        return max(1, sum(len(g['params']) for g in self.param_groups)) * _ITEM.size

    def _upload(self, live, capturing):
        wo = self._wo
        copies = wo.copies if wo is not None else {}
        rows, begin = [], 0
        for p, g, st, gi in live:
            ent = copies.get(id(p))
            if ent is not None:
                w, wt = ent
                N, K = w.shape
                tiles_k = (K + 63) // 64
                blocks = ((N + 63) // 64) * tiles_k
                wp, wtp = w.data_ptr(), wt.data_ptr()
            else:
                N = K = tiles_k = wp = wtp = 0
                blocks = (p.numel() + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK
            if blocks == 0:
                continue
            rows.append(_ITEM.pack(p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['step'].data_ptr(),
                                   wp, wtp, p.numel(), N, K, begin, tiles_k, gi, 0, 1.0, 1.0))
            begin += blocks
        assert begin < 2 ** 31
        cap = self._capacity()
        stage, self._spare = self._spare, None
        if stage is None or stage.numel() < cap:
            if capturing:
                raise RuntimeError('FusedAdam: no pinned staging buffer is ready for an upload inside a graph capture (pinned memory must not be '
                                   'allocated there); call reserve_staging() before each capture after the first')
            stage = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        if self._table is None or self._table.numel() < cap:
            self._table = torch.empty(cap, dtype=torch.uint8, device=self._device)
        blob = b''.join(rows)
        if blob:
            stage[:len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
            self._table[:len(blob)].copy_(stage[:len(blob)], non_blocking=True)
        if capturing:
            self._graph_staging.append(stage)               # the graph's copy node reads this memory at every replay
        else:
            self._staging = stage                            # the previous buffer goes back to torch's pinned cache, which waits for its copy
            self.reserve_staging()
        self._n_items, self._blocks = len(rows), begin

    def reserve_staging(self):
        """Keep one pinned staging buffer ready: an upload recorded inside a graph capture takes it, because pinned memory must not be allocated
        there.  Every eager upload leaves one behind, so the first capture after an eager step needs no call; call this (outside a capture)
        before any further capture that no eager step precedes.  ``capture_update_step`` does."""
        cap = self._capacity()
        if self._spare is None or self._spare.numel() < cap:
            self._spare = torch.empty(cap, dtype=torch.uint8, pin_memory=True)

    def release_graph_staging(self):
        """Each captured step keeps its staging buffer (one table, ~100 B per parameter) for as long as this optimizer lives, because the optimizer
        cannot know when a graph dies.  A caller that has dropped EVERY graph that recorded a step of this optimizer may hand them back here."""
        self._graph_staging.clear()

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        if self._wo is not None and self._wo.stale():           # parameter storage replaced: back to flat items, refresh() does the copies
            self.detach_operands()
        live, key = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if not g.is_cuda or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                    raise RuntimeError('FusedAdam needs dense contiguous fp32 device gradients of the parameter\'s shape (got %s %s on %s)'
                                       % (g.dtype, tuple(g.shape), g.device))
                st = self.state[p]
                if len(st) == 0:
                    if capturing:
                        raise RuntimeError('FusedAdam: optimizer state would be created inside a graph capture (its zero fill would be replayed); '
                                           'run a warm-up step first')
                    st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                live.append((p, g, st, gi))
                key.append((p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['step'].data_ptr(), gi))
        if not live:
            return loss
        self.sync_hyperparameters()
        with torch.cuda.device(self._device):
            # a captured step always records its own upload: the replay then does not depend on what eager steps wrote into the table since
            if capturing or key != self._key:
                self._upload(live, capturing)
                self._key = None if capturing else key       # a recorded upload has not run: the table still holds the last eager one
            if self._n_items:
                L.adam_advance(self._table, self._n_items, self._hyper)
                L.adam_step(self._table, self._n_items, self._blocks, self._hyper)
        self._updated = [p for p, _, _, _ in live]
        self.mark_updated()
        return loss

    def mark_updated(self):
        """Host-side bookkeeping of one executed update: bump ``_version`` of every parameter the last step() updated (every version-keyed weight
        cache of the library then rebuilds) and mark the attached operand copies current.  step() calls it; after ``graph.replay()`` of a captured
        step, call it yourself (``capture_update_step``'s replay does)."""
        wo = self._wo
        was_current = wo is not None and wo.versions == [p._version for p in wo.params]
        torch.autograd.graph.increment_version(self._updated)
        if wo is not None:
            done = {id(p) for p in self._updated}
            # every copy is either rewritten by this update or was current and belongs to a parameter nobody touched
            if was_current or all(id(p) in done for p in wo.params):
                wo.mark_current()
