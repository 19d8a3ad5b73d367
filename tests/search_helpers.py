"""What the search tests share: the exhaustive answer csm_search_windows
must return (test-only)."""
import numpy as np


def reduce_best(sc, flat, n_cand):
    gidx = np.arange(sc.size, dtype=np.int64) * n_cand + flat.astype(np.int64)
    best = sc.max()
    k = int(np.argmin(np.where(sc == best, gidx, np.iinfo(np.int64).max)))
    return k, gidx[k]


def check_same(ctx, pts, p, gi, centers, **kw):
    """search_windows == reduced best_windows; returns (best, window, stats)."""
    import roborts_csm
    na, ns = roborts_csm.window_dims(p)
    sc, flat, x, y, a = ctx.best_windows(pts, p, gi, centers)
    k, _ = reduce_best(sc, flat, na * ns * ns)
    b, w, st = ctx.search_windows(pts, p, gi, centers, **kw)
    assert w == k, (w, k, st)
    assert b.score == sc[k] and b.flat_index == flat[k], (b.score, sc[k], b.flat_index, flat[k])
    assert b.x == x[k] and b.y == y[k] and b.angle == a[k]
    return b, w, st
