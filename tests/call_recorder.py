"""The generic half of the call-recording tests (a plain helper module, not collected by pytest).  ``Recorder`` wraps every public function of
``whmr_amd._lib``: each top-level call is snapshotted (inputs cloned on the current stream), run, and handed to the subclass's ``on_<name>``
handler right away; a call with no handler, or with a flag its handler does not allow, fails the test.  The handlers, the expected call counts
and the bounds live in the tests (test_vit_train_bf16_calls_gpu.py, test_vit_blocked_bf16_calls_gpu.py)."""
import collections
import inspect

import torch

# pure helpers: no kernel of their own (or only reached nested inside a checked call)
ALLOW = {'lib', 'gemm_tn_ok', 'gemm_tn_group_ok', 'splitk_workspace', 'zero_page', 'train_scratch', 'side_stream',
         'struct_format'}     # (struct_format: the ctypes layouts as struct strings, called when whmr_amd.train is first imported inside a forward)
# public classes of _lib: ctypes descriptors, and WeightOperands (its refresh() calls the library directly; the copies are checked after the step)
CLASSES = {'WhmrGemm', 'WhmrGemmBlk', 'WhmrGemmBlkMx', 'WhmrSmplModel', 'WhmrStageTail', 'WhmrMafWeights', 'WhmrTnItem', 'WeightOperands',
           'ClockProbe'}


def _snap(v):
    if isinstance(v, torch.Tensor):
        return v.clone()
    if isinstance(v, (list, tuple)):
        return type(v)(_snap(x) for x in v)
    if isinstance(v, dict):
        return {k: _snap(x) for k, x in v.items()}
    return v


class Recorder:
    def __init__(self, L):
        self.L, self.depth, self.counts, self.worst = L, 0, collections.Counter(), {}
        self.sigs = {}
        self.result = None                  # what the call being handled returned

    def install(self, monkeypatch):
        L = self.L
        for name, fn in list(vars(L).items()):
            if name.startswith('_') or not callable(fn):
                continue
            if inspect.isclass(fn):
                assert name in CLASSES, 'new public class in _lib without a decision in this test: %s' % name
                continue
            if not inspect.isfunction(fn) or fn.__module__ != L.__name__:
                continue
            self.sigs[name] = inspect.signature(fn)
            monkeypatch.setattr(L, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*args, **kwargs):
            if self.depth > 0 or name in ALLOW:
                self.depth += 1
                try:
                    return fn(*args, **kwargs)
                finally:
                    self.depth -= 1
            handler = getattr(self, 'on_' + name, None)
            assert handler is not None, 'top-level call of _lib.%s has no float64 reference' % name
            b = self.sigs[name].bind(*args, **kwargs)
            b.apply_defaults()
            live = dict(b.arguments)
            snap = {k: _snap(v) for k, v in live.items()}
            self.depth += 1
            try:
                out = fn(*args, **kwargs)
            finally:
                self.depth -= 1
            self.counts[name] += 1
            self.result = out
            handler(live, snap)
            self.result = None
            return out
        return call

    def record(self, key, ratio):
        assert ratio <= 1.0, '%s: error exceeds its derived bound (worst ratio %.3g)' % (key, ratio)
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)

    @staticmethod
    def _only(live, allowed, defaults):
        for k, v in live.items():
            if k in allowed:
                continue
            d = defaults[k].default
            assert v is d or (v is not None and d is not None and not isinstance(v, torch.Tensor) and v == d), \
                'flag %s=%r is not modelled by the reference' % (k, v)

    def table(self):
        return ['  %-52s %.3e' % (k, self.worst[k]) for k in sorted(self.worst)]
