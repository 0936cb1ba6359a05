"""Optimiser and learning-rate schedule of the reference, on the flat parameter buffer.

`tf.train.AdamOptimizer` / `tf.train.MomentumOptimizer` through `slim.learning.create_train_op` (reference
src/model_base.py:387-401, :852-883) with the TF-1.9 ApplyAdam formula (eps outside the
bias correction), L2 regularisation over every trainable variable
(model_base.py:408-417, common/ops.py:184-190) folded into the update as grad += decay*w,
and the cosine schedule of `_create_cosine_lr` (model_base.py:809-820).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from .prune import PruneMask, PruneSpec, prune_sparsity_at  # noqa: F401  (the schedule is part of this module's interface)


def cosine_lr(step, max_step, lr_start, lr_end):
    s = np.float32(step / max_step)
    s = np.float32(1.0) + np.cos(np.minimum(np.float32(1.0), s) * np.float32(math.pi), dtype=np.float32)
    return float(np.float32(np.float32(lr_start - lr_end) * s / np.float32(2) + np.float32(lr_end)))


def legacy_lr_reduce(lr, epoch, lr_end, every_n_epochs):
    """train_fn._lr_reduce_check (src/train_fn.py:307-317)."""
    if lr > lr_end and epoch % every_n_epochs == 0:
        lr = max(lr / 2, lr_end)
    return lr


def ema_rate(decay, t):
    """tf.train.ExponentialMovingAverage(decay, num_updates=n).apply(): the decay of one shadow update is
    min(decay, (1 + n) / (10 + n)), so that the average warms up; n = t - 1 for the optimiser's count t AFTER step() has
    incremented it (the t of lr_t), i.e. the number of updates applied before this one."""
    n = t - 1
    return min(float(decay), (1.0 + n) / (10.0 + n))


class GradClip:
    """`--clip_gradient_norm c` (train.py:137 -> model_base.py:394-401): slim.learning.create_train_op clips EVERY variable's
    gradient by that tensor's own norm (clip_gradient_norms -> tf.clip_by_norm [TF-1.9 slim]), after the gradient
    multipliers; the L2 term is part of the loss and therefore of the clipped gradient.  One chunk table per flat
    parameter buffer (comic_clip_by_norm, include/comic_hip.h)."""
    CHUNK = 8192

    def __init__(self, params, clip_norm):
        import torch
        self.lib = L.load()
        self.clip_norm = float(clip_norm)
        rows = []
        for seg, k in enumerate(params.shapes):
            n = int(np.prod(params.shapes[k])) if len(params.shapes[k]) else 1
            first, count = len(rows), (n + self.CHUNK - 1) // self.CHUNK
            for c in range(count):
                rows.append((seg, params.offsets[k] + c * self.CHUNK, min(self.CHUNK, n - c * self.CHUNK), first, count))
        self.n_chunks = len(rows)
        self.chunks = torch.from_numpy(np.asarray(rows, np.int64).reshape(-1, 5)).to(params.device)
        self.partial = torch.zeros(max(1, self.n_chunks), dtype=torch.float32, device=params.device)

    def apply(self, params, grads, l2, grad_scale, skip=None, mask=None):
        """mask (a prune.PruneMask): the gradients of pruned weights are zeroed first -- the norm of a variable must not count
        weights that no longer exist (one extra launch, in this combination only)."""
        st = skip if skip is not None else getattr(grads, 'status', None)
        if mask is not None:
            mask.mask_buffer(grads)
        L.check(self.lib.comic_clip_by_norm(grads.data.data_ptr(), params.data.data_ptr(), self.chunks.data_ptr(),
                                            self.n_chunks, l2, grad_scale, self.clip_norm, self.partial.data_ptr(),
                                            st.data_ptr() if st is not None else None, L.stream_ptr()), 'clip_by_norm')


class AdamTF:
    def __init__(self, params, beta1=0.9, beta2=0.999, epsilon=1e-2, l2_decay=1e-5, clip_norm=0.0, ema_decay=0.0,
                 prune=None):
        self.lib = L.load()
        self.params = params
        self.m = params.like()
        self.v = params.like()
        self.beta1, self.beta2, self.eps, self.l2 = beta1, beta2, epsilon, l2_decay
        self.t = 0                      # number of applied updates (== global_step)
        self.clip = GradClip(params, clip_norm) if clip_norm and clip_norm > 0 else None
        self._ema_init(ema_decay)
        self._prune_init(prune)

    def _prune_init(self, prune):
        """`prune` (a prune.PruneSpec or None): a bit mask over the flat buffer; the update launches are the masked forms
        (comic_*_tf_masked) and a mask event (comic_prune_select on w, m, v and the shadow) follows the update whose count is
        on the schedule.  None: no mask, the launches of the gated / EMA forms."""
        self.mask = PruneMask(self.params, prune) if prune is not None else None

    def prune_keep_zeros(self):
        """--prune_keep_zeros: freeze the zeros of the variables as they are now (call after the checkpoint is loaded)."""
        self.mask.from_zeros(self.m, self.v, self.ema)

    def _prune_event(self):
        if self.mask is not None and self.mask.spec.event_at(self.t):
            self.mask.event(self.t, self.m, self.v, self.ema)

    def _ema_init(self, ema_decay):
        """`--ema_decay d` (tf.train.ExponentialMovingAverage): a shadow of every variable, updated inside the update
        launch (comic_*_tf_ema) behind the same gate and ranges.  d = 0: no shadow, the launches of the gated forms."""
        self.ema_decay = float(ema_decay or 0.0)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError('ema_decay must be in [0, 1): %r' % (ema_decay,))
        self.ema = self.params.like() if self.ema_decay > 0 else None
        self.ema_reset()

    def ema_reset(self):
        """A shadow starts at its variable's value (TF: the initial value): call after the variables are in place."""
        if self.ema is not None:
            self.ema.flat.copy_(self.params.flat)

    def step(self, grads, lr, grad_scale=1.0, skip=None, ranges=None, before_range=None):
        """skip: the status word of ANOTHER gradient buffer that gates this update too (the CNN optimisers of cnn_finetune
        follow the decoder's verdict on the step: model.py).
        ranges: [(lo, hi), ...] element ranges of the flat buffer (together: all of it) updated one launch each, in that
        order, `before_range(i)` called in front of launch i -- the chunked gradient exchange (trainer.DataParallel.
        exchange_and_step) orders the stream behind chunk i's all-reduce there, so the update of a chunk runs beside the
        exchange of the next.  The update is element-wise: any partition gives the bits of the one-launch update."""
        self.t += 1
        lr_t = lr * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        # a gradient buffer with a status word (decoder.FlatParams(status_tail=True)): the update is skipped on the device
        # when comic_decoder_train_step voided the step (on any rank: the word is part of the all-reduced buffer).  The
        # host-side step count `t` advances regardless -- one bias-correction step of drift per voided step, and the run
        # stops at the next log point anyway (train_fn._check_loss reads the sticky count).
        st = skip if skip is not None else getattr(grads, 'status', None)
        if self.clip is not None:
            assert ranges is None, 'per-variable clipping reads whole variables: one launch over the flat buffer'
            self.clip.apply(self.params, grads, self.l2, grad_scale, skip=st, mask=self.mask)
        omd = 1.0 - ema_rate(self.ema_decay, self.t) if self.ema is not None else 0.0
        for i, (lo, hi) in enumerate(ranges or [(0, self.params.numel)]):
            if before_range is not None:
                before_range(i)
            if self.mask is not None:
                L.check(self.lib.comic_adam_tf_masked(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                      self.m.data.data_ptr() + 4 * lo, self.v.data.data_ptr() + 4 * lo, hi - lo,
                                                      lr_t, self.beta1, self.beta2, self.eps, self.l2, grad_scale,
                                                      st.data_ptr() if st is not None else None,
                                                      self.ema.data.data_ptr() + 4 * lo if self.ema is not None else None, omd,
                                                      self.mask.words.data_ptr(), lo, L.stream_ptr()), 'adam_tf_masked')
                continue
            if self.ema is not None:
                L.check(self.lib.comic_adam_tf_ema(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                   self.m.data.data_ptr() + 4 * lo, self.v.data.data_ptr() + 4 * lo, hi - lo,
                                                   lr_t, self.beta1, self.beta2, self.eps, self.l2, grad_scale,
                                                   st.data_ptr() if st is not None else None,
                                                   self.ema.data.data_ptr() + 4 * lo, omd, L.stream_ptr()), 'adam_tf_ema')
                continue
            L.check(self.lib.comic_adam_tf_gated(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                 self.m.data.data_ptr() + 4 * lo, self.v.data.data_ptr() + 4 * lo, hi - lo,
                                                 lr_t, self.beta1, self.beta2, self.eps, self.l2, grad_scale,
                                                 st.data_ptr() if st is not None else None, L.stream_ptr()), 'adam_tf')
        self._prune_event()     # behind every range's update, on the step's stream

    def state_dict(self):
        sd = dict(t=self.t, m=self.m.data.clone(), v=self.v.data.clone())
        if self.ema is not None:
            sd['ema'] = self.ema.data.clone()
        if self.mask is not None:
            sd['prune_mask'] = self.mask.words.clone()
        return sd

    def load_state_dict(self, sd):
        self.t = int(sd['t'])
        self.m.data.copy_(sd['m'])
        self.v.data.copy_(sd['v'])
        if self.ema is not None and 'ema' in sd:
            self.ema.data.copy_(sd['ema'])
        if self.mask is not None and 'prune_mask' in sd:
            self.mask.words.copy_(sd['prune_mask'])


class MomentumTF:
    """tf.train.MomentumOptimizer(lr, momentum=0.9, use_nesterov=False) (reference src/model_base.py:867-880;
    `--optimiser sgd`): accum = momentum*accum + g, w -= lr*accum, with the same L2 fold as AdamTF.  Same interface
    (`t`, `step`, `m` = the accumulator; `v` stays zero so checkpoints keep one layout)."""

    def __init__(self, params, momentum=0.9, l2_decay=1e-5, clip_norm=0.0, ema_decay=0.0, prune=None, **_):
        self.lib = L.load()
        self.params = params
        self.m = params.like()
        self.v = params.like()
        self.momentum, self.l2 = momentum, l2_decay
        self.beta1, self.beta2, self.eps = momentum, 0.0, 0.0
        self.t = 0
        self.clip = GradClip(params, clip_norm) if clip_norm and clip_norm > 0 else None
        self._ema_init(ema_decay)
        self._prune_init(prune)

    _ema_init = AdamTF._ema_init
    ema_reset = AdamTF.ema_reset
    _prune_init = AdamTF._prune_init
    _prune_event = AdamTF._prune_event
    prune_keep_zeros = AdamTF.prune_keep_zeros

    def step(self, grads, lr, grad_scale=1.0, skip=None, ranges=None, before_range=None):
        """ranges / before_range: as AdamTF.step."""
        self.t += 1
        st = skip if skip is not None else getattr(grads, 'status', None)
        if self.clip is not None:
            assert ranges is None, 'per-variable clipping reads whole variables: one launch over the flat buffer'
            self.clip.apply(self.params, grads, self.l2, grad_scale, skip=st, mask=self.mask)
        omd = 1.0 - ema_rate(self.ema_decay, self.t) if self.ema is not None else 0.0
        for i, (lo, hi) in enumerate(ranges or [(0, self.params.numel)]):
            if before_range is not None:
                before_range(i)
            if self.mask is not None:
                L.check(self.lib.comic_momentum_tf_masked(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                          self.m.data.data_ptr() + 4 * lo, hi - lo, lr, self.momentum, self.l2,
                                                          grad_scale, st.data_ptr() if st is not None else None,
                                                          self.ema.data.data_ptr() + 4 * lo if self.ema is not None else None,
                                                          omd, self.mask.words.data_ptr(), lo, L.stream_ptr()),
                        'momentum_tf_masked')
                continue
            if self.ema is not None:
                L.check(self.lib.comic_momentum_tf_ema(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                       self.m.data.data_ptr() + 4 * lo, hi - lo, lr, self.momentum, self.l2,
                                                       grad_scale, st.data_ptr() if st is not None else None,
                                                       self.ema.data.data_ptr() + 4 * lo, omd, L.stream_ptr()),
                        'momentum_tf_ema')
                continue
            L.check(self.lib.comic_momentum_tf_gated(self.params.data.data_ptr() + 4 * lo, grads.data.data_ptr() + 4 * lo,
                                                     self.m.data.data_ptr() + 4 * lo, hi - lo, lr, self.momentum, self.l2,
                                                     grad_scale, st.data_ptr() if st is not None else None, L.stream_ptr()),
                    'momentum_tf')
        self._prune_event()

    state_dict = AdamTF.state_dict
    load_state_dict = AdamTF.load_state_dict


def make_optimiser(name, params, epsilon=1e-2, l2_decay=1e-5, clip_norm=0.0, ema_decay=0.0, prune=None):
    """`_get_optimiser` (model_base.py:852-883) + create_train_op's clip_gradient_norm (model_base.py:394-401);
    ema_decay > 0: a tf.train.ExponentialMovingAverage shadow of the variables (`opt.ema`); prune (a prune.PruneSpec):
    gradual magnitude pruning of the variables it names (`opt.mask`)."""
    if name == 'adam':
        return AdamTF(params, epsilon=epsilon, l2_decay=l2_decay, clip_norm=clip_norm, ema_decay=ema_decay, prune=prune)
    if name == 'sgd':
        return MomentumTF(params, l2_decay=l2_decay, clip_norm=clip_norm, ema_decay=ema_decay, prune=prune)
    raise ValueError('Unknown optimiser.')
