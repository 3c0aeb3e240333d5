"""The numpy oracle of the decoded-mode TBPTT loss (``sur_tbptt_decoded_loss``, ``sur_latent_deltas``: include/surrogate_hip.h),
shared by tests/test_sur_decoded_host.py and tests/test_sur_decoded_gpu.py.  Nothing in here needs a GPU.

Elementwise values are fp32 numpy expressions, one rounding per operation (numpy never contracts a multiply with an add);
every sum is fp64.  The helpers of tests/_sur_tail_oracle.py (guards, bit views, ``rel_err``, the observation log) are reused
by import."""
import numpy as np

from _sur_tail_oracle import U, bits, guarded, rel_err  # noqa: F401


def decoded_loss_oracle(states, out_all, delta, mean, stdv, order=0):
    """states [B, T, N] fp32 (any strides), out_all [T, B, N] fp32 (row T-1 is not read).  With prev[b, 0] = states[b, 0] and
    prev[b, t] = out_all[t-1, b]:
      fp32  outdeltas, deltas [B, T-1, N]; dout_all [T, B, N] (row T-1 zero); the error and its square
      fp64  loss, hsteploss [T], stats = (mean, unbiased std) of outdeltas, then of deltas
    ``order`` 1 sums the same terms in another order (reversed, row by row)."""
    s, o = np.asarray(states), np.asarray(out_all)
    assert s.dtype == np.float32 and o.dtype == np.float32
    B, T, N = s.shape
    f = np.float32
    ob = o[:T - 1].transpose(1, 0, 2)                                   # [B, T-1, N]: out_all[t, b] at [b, t]
    prev = np.concatenate((s[:, :1], ob), axis=1)                       # [B, T, N]
    err = prev - s
    sq = err * err
    od = ((ob - prev[:, :T - 1]) / f(delta) - f(mean)) / f(stdv)
    dl = ((s[:, 1:] - s[:, :-1]) / f(delta) - f(mean)) / f(stdv)
    count = float(B * T * N)
    dout = np.zeros((T, B, N), dtype=np.float32)
    dout[:T - 1] = (f(2.0 / count) * (ob - s[:, 1:])).transpose(1, 0, 2)
    assert err.dtype == sq.dtype == od.dtype == dl.dtype == np.float32

    def total(x, axis=None):
        x = x.astype(np.float64)
        steps = x.shape[1]
        if order == 0:
            return np.add.reduce(x.transpose(1, 0, 2).reshape(steps, -1), axis=1) if axis == "t" else float(np.sum(x))
        x = x[::-1, :, ::-1]
        return np.array([np.sum(x[:, t].ravel()) for t in range(steps)]) if axis == "t" else float(np.sum(np.sum(x, axis=2)))

    dcount = float(B * (T - 1) * N)

    def mean_std(x):
        x64 = x.astype(np.float64)
        s1, s2 = total(x), total(x64 * x64 if order == 0 else x * x.astype(np.float64))
        m = s1 / dcount
        return m, float(np.sqrt(max(s2 - dcount * m * m, 0.0) / (dcount - 1.0)))

    m_od, s_od = mean_std(od)
    m_dl, s_dl = mean_std(dl)
    return dict(outdeltas=od, deltas=dl, dout_all=dout, loss=total(sq) / count, hsteploss=total(sq, "t") / float(B * N),
                stats=np.array([m_od, s_od, m_dl, s_dl]))


def latent_deltas_oracle(state0, out_all, delta, mean, stdv):
    """d_all [K, B, N] fp32 of ``sur_latent_deltas``: state0 [B, N], out_all [K, B, N]."""
    o, f = np.asarray(out_all), np.float32
    prev = np.concatenate((np.asarray(state0)[None], o[:-1]), axis=0)
    d = ((o - prev) / f(delta) - f(mean)) / f(stdv)
    assert d.dtype == np.float32
    return d


def decoded_inputs(B, T, N, seed, storage="batch"):
    """states [B, T, N] (a view of the storage asked for) and out_all [T, B, N] with out_all[t] = states[:, t+1] + 0.1 normal
    (row T-1, which has no target, is the last state + noise), fp32."""
    rs = np.random.RandomState(seed)
    if storage == "batch":
        states = rs.uniform(-1, 1, (B, T, N)).astype(np.float32)
    elif storage == "time":
        states = rs.uniform(-1, 1, (T, B, N)).astype(np.float32).transpose(1, 0, 2)
    else:                                                              # padded strides
        states = rs.uniform(-1, 1, (B, T + 2, N + 5)).astype(np.float32)[:, 1:T + 1, 2:N + 2]
    target = np.concatenate((states[:, 1:], states[:, -1:]), axis=1).transpose(1, 0, 2)
    out_all = (target + np.float32(0.1) * rs.standard_normal((T, B, N)).astype(np.float32)).astype(np.float32)
    return states, np.ascontiguousarray(out_all)
