"""Float64 reference of the moving-average shadow of `--ema_decay` (tests/test_ema_cpu.py, tests/test_gpu_ema.py):
tf.train.ExponentialMovingAverage(decay, num_updates).apply() after the optimiser's update,

    decay_t = min(decay, (1 + n) / (10 + n)),   n = updates applied before this one
    shadow  = shadow - (1 - decay_t) * (shadow - var)          (var: the UPDATED variable)

written independently of optim.ema_rate: `rate` is the closed form below, `update` one application on the values the
device itself produced, `replay` the recurrence over a recorded trajectory of the variables."""
import numpy as np

EMA_TOL = 1e-6          # the bound of test_momentum_tf_matches_oracle: one subtract, one multiply-add per element


def rate(decay, t):
    """The decay of update number t (1-based: the optimiser's count after it has incremented it)."""
    warm_up = t / (9.0 + t)                 # (1 + (t - 1)) / (10 + (t - 1))
    return decay if decay < warm_up else warm_up


def update(shadow, w_new, omd):
    """One shadow update in float64 on float32 operands; omd as the float32 the host passes to the kernel."""
    s = np.asarray(shadow, np.float64)
    return s + (np.asarray(w_new, np.float64) - s) * np.float64(np.float32(omd))


def replay(w0, trajectory, decay):
    """w0: the variables the shadow starts from; trajectory: the variables after update 1, 2, ... -> the final shadow
    (float64), every step's factor rounded to float32 like the kernel's argument."""
    s = np.asarray(w0, np.float64).copy()
    for t, w in enumerate(trajectory, 1):
        s = update(s, w, 1.0 - rate(decay, t))
    return s
