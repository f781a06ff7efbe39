"""
param_pool.py -- all variables of a network in ONE flat fp32 buffer.

`ParamPool` is the one owner of that idea for every trainable network of the package (engine.ConvStack is one; the
EnhanceNet generator and discriminator hold one each): the layout, the gradient buffer and the optimizer slots that mirror
it, the step count, the optimizer launches on the flat buffers, the TensorFlow-checkpoint walk and the data-parallel
levelling.  One layout means the optimizer is one launch and the data-parallel exchange ONE all-reduce of `grads`.

A captured train step (engine.ConvStack.train_step_replay) holds the ADDRESSES of `params`, `grads`, `opt_m` and `opt_v`:
a restore writes into the buffers that exist, and dropping a slot tells the owner (`on_slot_dropped`).
"""
import numpy as np
import torch

from . import ops

_IDENTITY = (lambda t: t, lambda a, like: a)


class ParamPool(object):
    def __init__(self, entries, device):
        """entries: [(name, shape)] or [(name, shape, (to_tf, from_tf))] in creation order.  `name` is the TensorFlow
        variable name.  Every variable starts on a 16-byte boundary: offsets start at 0 and every length is rounded up to
        4 floats (`state_dict()` files store the flat buffer, so this layout is a file format).  to_tf(view) gives the
        variable in TensorFlow's layout, from_tf(tensor, like=view) the reverse; without the pair both are the identity."""
        self.device = torch.device(device)
        # per variable (name, offset, length, shape, to_tf, from_tf): plain tuples, view() unpacks one on every call of the
        # eager train steps (ESPCN's is host-bound within a few microseconds)
        self.entries, off = [], 0
        for name, shape, *convert in entries:
            n = int(np.prod(shape, dtype=np.int64))
            self.entries.append((name, off, n, tuple(shape)) + (convert[0] if convert else _IDENTITY))
            off += (n + 3) // 4 * 4
        self.flat_size = off
        self.num_params = sum(n for _, _, n, _, _, _ in self.entries)
        self.params = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.opt_m, self.opt_v = None, None     # Adam m, v / the Momentum accumulator: None until an optimizer or a restore needs them
        self.t = 0                              # optimizer steps taken
        self.on_slot_dropped = None             # optional fn(): the owner's captured steps point at a slot that is gone
        self._adam_state = None                 # ops.adam_state(): {int64 t; float lr; ...} on the device
        self._state_t, self._state_lr = None, None    # host mirror of what the device block holds

    def view(self, j, buf=None):
        """Variable j of `buf` (params, grads or a slot), computed from the buffer at call time."""
        _, off, n, shape, _, _ = self.entries[j]
        return (self.params if buf is None else buf)[off:off + n].view(shape)

    def names(self):
        return [name for name, _, _, _, _, _ in self.entries]

    def layout(self):
        return [(name, off, shape) for name, off, _, shape, _, _ in self.entries]

    def variables(self, buf=None):
        """{tf variable name: the variable in TensorFlow's layout} of params (or of `buf`); a view where the layouts agree."""
        return {name: to_tf(self.view(j, buf)) for j, (name, _, _, _, to_tf, _) in enumerate(self.entries)}

    # ---- the slot rules -------------------------------------------------------------------------
    def _new_slot(self):
        return torch.zeros_like(self.params)

    def ensure_slots(self, count):
        """The slots an optimizer needs exist: Adam two, Momentum one."""
        if self.opt_m is None:
            self.opt_m = self._new_slot()
        if count == 2 and self.opt_v is None:
            self.opt_v = self._new_slot()

    def restore_slot(self, attr, fill):
        """Restores `opt_m` / `opt_v` IN PLACE: `fill(buf)` writes into the buffer that exists; one is allocated only when
        there is none yet (no captured step can hold a slot that never existed: capturing allocates them first)."""
        if getattr(self, attr) is None:
            setattr(self, attr, self._new_slot())
        fill(getattr(self, attr))

    def drop_second_slot(self):
        """A Momentum state restored over Adam slots: `opt_m` now holds the accumulator and `opt_v` has no meaning.  It
        is released and the owner told (every captured step goes: an Adam step among them would write to it)."""
        if self.opt_v is not None:
            self.opt_v = None
            if self.on_slot_dropped is not None:
                self.on_slot_dropped()

    # ---- optimizers: one launch over the flat buffers -------------------------------------------
    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """tf.train.AdamOptimizer(...).minimize(loss)."""
        self.ensure_slots(2)
        self.t += 1
        ops.adam_tf_step(self.params, self.grads, self.opt_m, self.opt_v, lr, self.t, beta1, beta2, eps)

    def momentum_clip_step(self, lr, momentum=0.9, gradient_cap=0.01):
        """vdsr/vdsr/model_vdsr.py:158-184: clip every gradient element to +-gradient_cap/lr, then Momentum."""
        self.ensure_slots(1)
        self.t += 1
        ops.momentum_clip_step(self.params, self.grads, self.opt_m, lr, momentum, gradient_cap / lr)

    def sync_adam_state(self, lr):
        """The device block {t, lr} follows the host's step count (a checkpoint load, levelling) and the fed rate; written
        only when one of them changed."""
        if self._adam_state is None:
            self._adam_state = ops.adam_state(self.device, t=self.t, lr=lr)
            self._state_t, self._state_lr = self.t, float(lr)
        if self._state_t != self.t:
            ops.adam_state_set(self._adam_state, t=self.t)
            self._state_t = self.t
        if self._state_lr != float(lr):
            ops.adam_state_set(self._adam_state, lr=lr)
            self._state_lr = float(lr)

    def adam_launch_dev(self, beta1=0.9, beta2=0.999, eps=1e-8):
        """The launch of adam_step_dev alone (srx_adam_tf_step_dev: the step count and the rate are read from device
        memory, and the count is advanced there): what a captured step holds."""
        ops.adam_tf_step_dev(self.params, self.grads, self.opt_m, self.opt_v, self._adam_state, beta1, beta2, eps)

    def count_dev_step(self):
        """The host's side of one srx_adam_tf_step_dev launch (issued or replayed)."""
        self.t += 1
        self._state_t += 1

    def adam_step_dev(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """adam_step with no per-step kernel argument, so that the launch can sit in a replayed graph."""
        self.ensure_slots(2)
        self.sync_adam_state(lr)
        self.adam_launch_dev(beta1, beta2, eps)
        self.count_dev_step()

    # ---- TensorFlow checkpoints: the variables and their slots ----------------------------------
    def _slots(self):
        if self.opt_m is None:
            return ()
        if self.opt_v is None:
            return (('Momentum', 'opt_m'),)
        return (('Adam', 'opt_m'), ('Adam_1', 'opt_v'))

    def tf_tensors(self):
        """{checkpoint key: ndarray}: `<name>` and, when the slots exist, `<name>/Adam` + `<name>/Adam_1` or
        `<name>/Momentum`.  (The step count and the beta powers are named by the owner: they differ per model.)"""
        out = {}
        for suffix, buf in [('', self.params)] + [('/' + s, getattr(self, attr)) for s, attr in self._slots()]:
            out.update({k + suffix: v.detach().cpu().numpy() for k, v in self.variables(buf).items()})
        return out

    def load_variables(self, values, buf=None):
        """values: {name: array-like in TensorFlow's layout}, names as in variables() (a trailing ':0' is accepted);
        written in place into params (or `buf`)."""
        index = {name: j for j, name in enumerate(self.names())}
        for name, val in values.items():
            key = name[:-2] if name.endswith(':0') else name
            if key not in index:
                raise KeyError('unknown variable %r' % name)
            dst, (_, _, _, _, to_tf, from_tf) = self.view(index[key], buf), self.entries[index[key]]
            t = torch.as_tensor(np.asarray(val), dtype=torch.float32)
            if tuple(t.shape) != tuple(to_tf(dst).shape):
                raise ValueError('%s: shape %s != %s' % (name, tuple(t.shape), tuple(to_tf(dst).shape)))
            dst.copy_(from_tf(t, dst).to(self.device))

    def load_tf_tensors(self, values, what='checkpoint', with_optimizer=True):
        """The reverse of tf_tensors(), in place.  Every variable must be there; the slots are restored when all of a kind
        are (restore_slot), and a Momentum accumulator without `Adam_1` drops the second slot."""
        names = self.names()
        missing = [k for k in names if k not in values]
        if missing:
            raise KeyError('%s lacks variables %s' % (what, missing[:4]))
        self.load_variables({k: values[k] for k in names})
        if not with_optimizer:
            return
        has = lambda slot: all('%s/%s' % (k, slot) in values for k in names)
        fill = lambda slot: lambda buf: self.load_variables({k: values['%s/%s' % (k, slot)] for k in names}, buf)
        if has('Adam'):
            self.restore_slot('opt_m', fill('Adam'))
        if has('Adam_1'):
            self.restore_slot('opt_v', fill('Adam_1'))
        if has('Momentum'):
            self.restore_slot('opt_m', fill('Momentum'))
            if not has('Adam_1'):
                self.drop_second_slot()

    # ---- data parallelism -----------------------------------------------------------------------
    def level_from_rank0(self):
        """Every replica starts as rank 0: parameters, the step count and the optimizer slots (a rank that resumed from a
        different checkpoint -- or none -- would otherwise run a different number of steps and hang the collective).
        Which slots rank 0 holds decides which broadcasts follow, so that head goes out before any slot: the collectives
        are equal in number and order on every rank, whatever each rank held before."""
        from . import dist
        dist.broadcast_(self.params, 0)
        step, has_m, has_v = dist.broadcast_ints([self.t, self.opt_m is not None, self.opt_v is not None], self.params.device)
        self.t = step
        for flag, attr in ((has_m, 'opt_m'), (has_v, 'opt_v')):
            if flag:
                self.restore_slot(attr, lambda buf: dist.broadcast_(buf, 0))
            else:
                setattr(self, attr, None)
