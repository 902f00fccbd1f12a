"""The rivals rule (include/f1p.h "Rivals") in plain numpy, loops and all: the reference of tests/test_rivals_host.py and
tests/test_gpu_rivals.py."""
import numpy as np

XYVYAW, POSE, ST7 = 0, 1, 2
EMPTY = (0.0, 0.0, 0.0, 0.0, -1.0)


def columns(states, layout):
    """-> (x, y, v, h) of the three layouts"""
    s = np.asarray(states, dtype=np.float64)
    if layout == XYVYAW:
        return s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    if layout == POSE:
        return s[:, 0], s[:, 1], s[:, 3], s[:, 2]
    if layout == ST7:
        return s[:, 0], s[:, 1], s[:, 3], s[:, 4] + s[:, 6]
    raise ValueError("layout")


def rivals(states, layout, M, radius, reach=np.inf, min_speed=0.5, groups=None):
    """-> dict(obs [E, M, 5], pace [E], idx int32 [E, M])"""
    x, y, v, h = columns(states, layout)
    E = x.shape[0]
    g = np.zeros(E, np.int64) if groups is None else np.asarray(groups, dtype=np.int64).reshape(-1)
    assert g.shape == (E,)
    reach2 = np.float64(reach) * np.float64(reach)
    obs = np.empty((E, M, 5))
    obs[:] = EMPTY
    idx = np.full((E, M), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(E):
            if g[i] < 0:
                continue
            cand = []
            for j in range(E):
                if j == i or g[j] != g[i]:
                    continue
                dx = x[j] - x[i]
                dy = y[j] - y[i]
                d2 = dx * dx + dy * dy
                if not d2 > reach2:                             # a NaN d2 is a candidate
                    cand.append((j, d2))
            for m in range(min(M, len(cand))):                  # np.argmin, repeatedly: the first NaN, else the first minimum
                k = int(np.argmin(np.array([d for _, d in cand])))
                j = cand.pop(k)[0]
                idx[i, m] = j
                obs[i, m] = (x[j], y[j], v[j] * np.cos(h[j]), v[j] * np.sin(h[j]), radius)
        pace = 1.0 / np.maximum(np.abs(v), min_speed)
    return dict(obs=obs, pace=pace, idx=idx)


def example_obstacles(st, M, radius):
    """the host construction of examples/common.py opponent_runs, one race of all, st [E, 4] = (x, y, v, yaw) -> (obs [E, M, 5], near [E, M])"""
    E = st.shape[0]
    d = np.hypot(st[:, None, 0] - st[None, :, 0], st[:, None, 1] - st[None, :, 1]) + np.diag(np.full(E, np.inf))
    near = np.argsort(d, axis=1)[:, :M]
    o = st[near]
    return np.stack([o[:, :, 0], o[:, :, 1], o[:, :, 2] * np.cos(o[:, :, 3]), o[:, :, 2] * np.sin(o[:, :, 3]), np.full((E, M), radius)], 2), near
