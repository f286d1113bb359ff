"""FlatAdam: ``torch.optim.Adam`` over ONE flat parameter buffer, one kernel launch per step.

The training step is host-bound: torch's multi-tensor Adam over the model's 174 tensors, and the max |w|
read-backs the weight packs need after every update (params._lagged_prefetch: one ``_foreach_norm`` + ``stack`` per tensor group),
are a few hundred small launches.  ``strive_adam_flat`` (csrc/optim.hip) does the update of all parameters AND max |w| of every
tensor in one pass; this module is its optimiser: it moves the parameters into one flat fp32 buffer (``p.data`` become views, in
``model.parameters()`` order at running-``numel`` offsets: the layout of ``DataParallelTrainer.bucket`` and ``ops.GradSink``), keeps
``exp_avg`` / ``exp_avg_sq`` flat, and reads the gradients from a flat buffer of its own whose views it binds as ``p.grad`` -- or
from the trainer's bucket (``use_grad_buffer``), so that one buffer serves both and nothing is copied.

The arithmetic is that of ``torch.optim.Adam`` (single-tensor form; reference src/train_traffic.py:275-277 creates that optimiser),
and ``state_dict()`` / ``load_state_dict()`` speak its format, so a checkpoint of either class loads into the other.
"""
import torch

from . import _lib as L
from . import params as P


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise NotImplementedError('FlatAdam takes one parameter group (got %d)' % len(params))
        if amsgrad or maximize:
            raise NotImplementedError('FlatAdam implements neither amsgrad nor maximize')
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError('invalid Adam hyper-parameters')
        # the group keys of torch.optim.Adam in this torch version, so that a state dict of one class loads into the other
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError('FlatAdam takes one parameter group (got %d)' % len(self.param_groups))
        self.flat_params = list(self.param_groups[0]['params'])
        ps = self.flat_params
        if not ps:
            raise ValueError('FlatAdam got no parameters')
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.requires_grad:
                raise ValueError('FlatAdam takes trainable fp32 parameters on one device')
        self._offsets, off = [], 0
        for p in ps:
            self._offsets.append(off)
            off += p.numel()
        self.numel = off
        self._offsets.append(off)
        self.flat = torch.empty((self.numel,), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(ps, self._offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.step_count = 0                                   # a host integer: every parameter takes every step
        self._seg_off = torch.tensor(self._offsets, dtype=torch.int64).to(dev)
        # max |w| of every parameter tensor after the last step (params.py serves it to the weight packs while it is current)
        self.absmax_table = torch.zeros((len(ps),), dtype=torch.float32, device=dev)
        self.table_epoch = -1
        self.table_versions = None
        self._index_cache = {}
        self.use_grad_buffer(None)
        P.parameters_changed()                                # every p.data moved
        P.register_absmax_source(self)

    # ---- gradients ----
    def use_grad_buffer(self, buf):
        """Read the gradients from ``buf`` (a flat fp32 buffer of at least ``numel`` elements in the parameters' layout, e.g.
        ``DataParallelTrainer.bucket``) and bind its views as ``p.grad``; ``None``: a buffer of this optimiser's own."""
        if buf is None:
            buf = torch.zeros((self.numel,), dtype=torch.float32, device=self.flat.device)
        if buf.dtype != torch.float32 or buf.device != self.flat.device or buf.numel() < self.numel or not buf.is_contiguous():
            raise ValueError('the gradient buffer must be a contiguous fp32 buffer of >= %d elements on %s' % (self.numel, self.flat.device))
        self.grad_flat = buf[:self.numel]
        self._grad_views = [self.grad_flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.flat_params, self._offsets)]
        for p, v in zip(self.flat_params, self._grad_views):
            p.grad = v

    def zero_grad(self, set_to_none=False):
        """Zero the flat gradient buffer and bind its views again (they are never set to None: the views ARE the gradients)."""
        self.grad_flat.zero_()
        for p, v in zip(self.flat_params, self._grad_views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    # ---- the step ----
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        if group.get('amsgrad') or group.get('maximize'):
            raise NotImplementedError('FlatAdam implements neither amsgrad nor maximize')
        base, gbase = self.flat.data_ptr(), self.grad_flat.data_ptr()
        for i, p in enumerate(self.flat_params):
            o = 4 * self._offsets[i]
            if p.data_ptr() != base + o or p.device != self.flat.device or not p.is_contiguous():
                raise RuntimeError('FlatAdam: parameter %d (shape %s) no longer lives in the flat buffer (model.to(...), or p.data was '
                                   'replaced): create the optimiser after moving the model' % (i, tuple(p.shape)))
            g = p.grad
            if g is None:                                     # no gradient = a zero gradient (every parameter takes every step)
                self._grad_views[i].zero_()
                p.grad = self._grad_views[i]
            elif g.data_ptr() != gbase + o or not g.is_contiguous():
                self._grad_views[i].copy_(g)                  # a gradient that is not the bound view: the slow path
        from . import ops
        lib = ops._lib_for(self.flat)
        beta1, beta2 = group['betas']
        t = self.step_count + 1
        lib.call('strive_adam_flat', L.ptr(self.flat), L.ptr(self.grad_flat), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), self.numel,
                 float(group['lr']), float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']),
                 1.0 - float(beta1) ** t, 1.0 - float(beta2) ** t, L.ptr(self._seg_off), len(self.flat_params), L.ptr(self.absmax_table),
                 L.stream_ptr(self.flat))
        self.step_count = t
        # the kernel wrote the parameters behind autograd's back (no version counter moved): THIS call announces the update, and the
        # table it has just written is the one that is current in the new epoch
        self.table_epoch = P.parameters_changed()
        self.table_versions = [p._version for p in self.flat_params]
        return loss

    # ---- torch.optim.Adam's state format ----
    def _segments(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.flat_params, self._offsets)]

    def state_dict(self):
        """``torch.optim.Adam``'s format: per parameter ``step`` (a float32 scalar tensor), ``exp_avg``, ``exp_avg_sq`` -- copies,
        not views of the flat buffers."""
        # The base class serialises ``self.state``; this optimiser keeps no per-parameter state between calls (the moments are the
        # flat buffers), so the entries exist only for the duration of this call -- state-dict hooks see them, step hooks never do.
        if self.step_count > 0:
            for p, m, v in zip(self.flat_params, self._segments(self.exp_avg), self._segments(self.exp_avg_sq)):
                self.state[p] = {'step': torch.tensor(float(self.step_count), dtype=torch.float32), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        """A state dict of ``torch.optim.Adam`` or of this class (``step`` a tensor or a plain integer)."""
        if len(state_dict['param_groups']) != 1:
            raise NotImplementedError('FlatAdam takes one parameter group (got %d)' % len(state_dict['param_groups']))
        super().load_state_dict(state_dict)
        group = self.param_groups[0]
        if group.get('amsgrad') or group.get('maximize'):
            self.state.clear()
            raise NotImplementedError('FlatAdam implements neither amsgrad nor maximize')
        steps = set()
        with torch.no_grad():
            for p, m, v in zip(self.flat_params, self._segments(self.exp_avg), self._segments(self.exp_avg_sq)):
                st = self.state.get(p)
                if not st:
                    steps.add(0)
                    m.zero_()
                    v.zero_()
                    continue
                steps.add(int(st['step']))
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
        self.state.clear()
        if len(steps) != 1:
            raise NotImplementedError('FlatAdam keeps one step count for all parameters; the state dict holds %s' % sorted(steps))
        self.step_count = steps.pop()
        self.flat_params = list(group['params'])
        self.table_epoch = -1                                 # (the parameters did not change, but nothing is served across a load)

    # ---- max |w| source (params.py) ----
    def absmax_rows(self):
        """{params._lag_key of a parameter view: its row of the table}"""
        rows = self.__dict__.get('_rows')
        if rows is None:
            rows = self._rows = {(self.flat.data_ptr() + 4 * o, tuple(p.shape), str(p.device)): i
                                 for i, (p, o) in enumerate(zip(self.flat_params, self._offsets))}
        return rows

    def absmax_index(self, keys, rows):
        """int64 device tensor of the table rows ``rows`` of the tensor group ``keys``, cached per group"""
        idx = self._index_cache.get(keys)
        if idx is None:
            idx = P.upload(torch.tensor(rows, dtype=torch.int64), self.flat.device)
            self._index_cache[keys] = idx
        return idx

    def absmax_current(self, i, t):
        """Is row ``i`` of the table max |t| right now: no parameter update has been announced since the step that wrote it, and no
        in-place operation has touched the tensor."""
        return self.table_epoch == P.param_epoch() and self.table_versions is not None and t._version == self.table_versions[i]

