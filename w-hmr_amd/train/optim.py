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

The gradient guard (off by default; the reference does not clip, trainer.py:112-117 is a bare Adam): ``max_grad_norm`` and ``skip_nonfinite`` are
attributes of the optimizer -- NOT keys of ``param_groups`` / ``defaults``, so ``state_dict()`` stays torch's -- pushed to the device like ``lr``.  A
guarded step is three launches (whmr_adam_grad_sumsq, whmr_adam_guard_advance, whmr_adam_step_guarded): the global L2 norm of the gradients the
table points at, then ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` + Adam, with two differences by design:

* ``p.grad`` is NOT rewritten: the update multiplies each gradient element by the coefficient on its way in (rounded to fp32 once, the value torch's
  in-place ``mul_`` would have left); writing it back would be 4 B per parameter of traffic for nothing.  Read ``clip_coef`` if you need it.
* with ``skip_nonfinite`` a step whose norm is NaN / Inf changes nothing on the device -- no p, exp_avg, exp_avg_sq, step count, bias correction or
  bf16 operand copy -- and the next good step is Adam step t + 1 of the steps APPLIED.  The host cannot know (it never reads), so its bookkeeping
  (``mark_updated()``: version bumps) runs regardless: a skipped step costs the version-keyed weight caches one spurious rebuild.

``grad_norm`` / ``clip_coef`` / ``steps_skipped`` / ``steps_seen`` are views into one persistent device buffer that every guarded step, eager or
replayed, writes: a loop may ``torch.stack`` them into a log without synchronising; ``guard_summary()`` is the one host read.  The counters are not
part of ``state_dict()``.

The library's weight caches are keyed on ``Parameter._version`` (models/*: ``_wcache``, L.WeightOperands); torch's in-place update bumps it, a
raw kernel does not, so ``step()`` calls ``torch.autograd.graph.increment_version`` on every parameter it updated (and ``mark_updated()`` does the
same after a graph replay, where no Python of ``step()`` runs).
"""
import math
import struct

import torch

from .. import _lib as L

# the packed rows of the device tables (include/whmr_hip.h; layouts: the ctypes mirrors of _lib)
_ITEM = struct.Struct(L.struct_format(L._WhmrAdamItem))
_HYPER = struct.Struct(L.struct_format(L._WhmrAdamHyper))                   # betas and lr as doubles (1 - beta, 1 - beta^t and lr / bc1 are formed in double on the device)
_GUARD_CFG = struct.Struct(L.struct_format(L._WhmrAdamGuardCfg))           # max_norm (<= 0: no clipping), skip_nonfinite, pad
_GUARD_STATE = struct.Struct(L.struct_format(L._WhmrAdamGuardState))       # grad_norm, clip_coef, apply, pad, steps_seen, steps_skipped


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, differentiable=False,
                 max_grad_norm=None, skip_nonfinite=False):
        for name, value in (('amsgrad', amsgrad), ('maximize', maximize), ('differentiable', differentiable)):
            if value:
                raise ValueError('FusedAdam implements plain Adam only: %s is not supported' % name)
        self._max_grad_norm, self._skip_nonfinite = self._check_guard(max_grad_norm, skip_nonfinite)
        self._guard_cfg = self._guard_cfg_staging = self._guard_pushed = None
        self._guard_state = self._partials = None
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

    @staticmethod
    def _check_guard(max_grad_norm, skip_nonfinite):
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, (torch.Tensor, bool)) or not isinstance(max_grad_norm, (int, float)):
                raise ValueError('FusedAdam: max_grad_norm is None or a Python float (got %r)' % (max_grad_norm,))
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
                raise ValueError('FusedAdam: max_grad_norm must be None or a finite float > 0 (got %r); the norm is the L2 norm' % max_grad_norm)
        return max_grad_norm, bool(skip_nonfinite)

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

    # ------------------------------------------------------------------ gradient guard
    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @property
    def skip_nonfinite(self):
        return self._skip_nonfinite

    @property
    def guarded(self):
        return self._max_grad_norm is not None or self._skip_nonfinite

    _KEEP = object()

    def set_grad_guard(self, max_grad_norm=_KEEP, skip_nonfinite=_KEEP):
        """Change the guard (an argument left out keeps its value; ``max_grad_norm=None`` stops clipping).  The device row follows at the next eager
        ``step()`` or ``sync_hyperparameters()`` -- between two replays of a captured guarded step that is the caller's line.  A step captured
        UNGUARDED stays unguarded: the guard's launches are not in that graph."""
        self._max_grad_norm, self._skip_nonfinite = self._check_guard(self._max_grad_norm if max_grad_norm is self._KEEP else max_grad_norm,
                                                                      self._skip_nonfinite if skip_nonfinite is self._KEEP else skip_nonfinite)

    def _guard_view(self, dtype, index):
        if self._guard_state is None:
            raise RuntimeError('FusedAdam: no guarded step has run yet (max_grad_norm / skip_nonfinite are off, or step() was not called)')
        return self._guard_state.view(dtype)[index]

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: global L2 norm of the gradients the last executed guarded step saw, before clipping.  No synchronisation."""
        return self._guard_view(torch.float32, 0)

    @property
    def clip_coef(self):
        """0-dim fp32 device tensor: the factor the last executed guarded step applied to every gradient (1.0 when it did not clip, 0.0 when it
        was skipped)"""
        return self._guard_view(torch.float32, 1)

    @property
    def steps_seen(self):
        """0-dim int64 device tensor: guarded steps executed so far, skipped ones included"""
        return self._guard_view(torch.int64, 2)

    @property
    def steps_skipped(self):
        """0-dim int64 device tensor: guarded steps that changed nothing because the norm was not finite"""
        return self._guard_view(torch.int64, 3)

    def guard_summary(self):
        """The guard's state as Python numbers.  This is the one host read: it synchronises with the device."""
        if self._guard_state is None:
            return dict(grad_norm=None, clip_coef=None, applied=None, steps_seen=0, steps_skipped=0)
        norm, coef, apply, _, seen, skipped = _GUARD_STATE.unpack(self._guard_state.cpu().numpy().tobytes())
        return dict(grad_norm=norm, clip_coef=coef, applied=bool(apply), steps_seen=seen, steps_skipped=skipped)

    def _guard_buffers(self, capturing):
        """the state buffer and the partial sums (one double per workgroup, sized like ``_table`` for every parameter rather than for this upload):
        created by the first eager guarded step, never inside a capture"""
        need = self._partials_capacity()
        if self._guard_state is not None and self._partials is not None and self._partials.numel() >= need:
            return
        if capturing:
            raise RuntimeError('FusedAdam: the gradient guard\'s device buffers would be created inside a graph capture (their fill would be replayed, '
                               'and a replay must write the buffer you read); run a warm-up step with the guard on first')
        if self._guard_state is None:
            self._guard_state = torch.zeros(_GUARD_STATE.size // 8, dtype=torch.int64, device=self._device)
            self._guard_state.view(torch.float32)[1] = 1.0
        if self._partials is None or self._partials.numel() < need:
            self._partials = torch.empty(need, dtype=torch.float64, device=self._device)

    def _partials_capacity(self):
        """workgroups of a table holding EVERY parameter (one double each): a step over fewer gradients, or after the operands were detached
        (tiles of a matrix are never fewer than its chunks), fits the same buffer"""
        copies = self._wo.copies if self._wo is not None else {}
        total = 0
        for group in self.param_groups:
            for p in group['params']:
                ent = copies.get(id(p))
                if ent is not None:
                    N, K = ent[0].shape
                    total += ((N + 63) // 64) * ((K + 63) // 64)
                else:
                    total += (p.numel() + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK
        return max(1, total)

    # ------------------------------------------------------------------ device rows
    def _rows(self):
        return [(float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay'])) for g in self.param_groups]

    def sync_hyperparameters(self):
        """Push lr / betas / eps / weight_decay of every group -- and the gradient guard's row -- to the device if they changed (on the current
        stream, no synchronisation).  An eager step() does this itself; between two replays of a captured step it is the caller's line after
        changing ``param_groups`` or calling ``set_grad_guard``."""
        self._sync_guard()
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

    def _sync_guard(self):
        """the guard's row, pushed as the hyper-parameter rows are.  Nothing exists, and nothing is pushed, until the guard is first switched on."""
        row = (self._max_grad_norm if self._max_grad_norm is not None else 0.0, int(self._skip_nonfinite))
        if row == self._guard_pushed or (self._guard_cfg is None and not self.guarded):
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdam: the gradient guard changed inside a graph capture; the recorded copy would reset it at every replay -- '
                               'run a warm-up step (or sync_hyperparameters()) before the capture')
        with torch.cuda.device(self._device):
            if self._guard_cfg is None:
                self._guard_cfg = torch.zeros(_GUARD_CFG.size, dtype=torch.uint8, device=self._device)
            self._guard_cfg_staging = torch.frombuffer(bytearray(_GUARD_CFG.pack(row[0], row[1], 0)), dtype=torch.uint8).pin_memory()   # fresh per push
            self._guard_cfg.copy_(self._guard_cfg_staging, non_blocking=True)
        self._guard_pushed = row

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
            if self.guarded:
                self._guard_buffers(capturing)
            # a captured step always records its own upload: the replay then does not depend on what eager steps wrote into the table since
            if capturing or key != self._key:
                self._upload(live, capturing)
                self._key = None if capturing else key       # a recorded upload has not run: the table still holds the last eager one
            if self._n_items and self.guarded:
                L.adam_grad_sumsq(self._table, self._n_items, self._blocks, self._partials)
                L.adam_guard_advance(self._table, self._n_items, self._hyper, self._partials, self._blocks, self._guard_cfg, self._guard_state)
                L.adam_step_guarded(self._table, self._n_items, self._blocks, self._hyper, self._guard_state)
            elif self._n_items:
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
