"""Shared by the lattice tests: the comparison bars against the oracle, and where a batch is cut -- the slices of the page-locked batch path,
the chunks of a pipelined plan, the ego ranges of MultiContext -- restated from the library's own formulas in ONE place, so that a threshold
change in the library shows up here and nowhere else."""
import numpy as np

from f1tenth_planning_amd.dist import shard_range

# f1p_lattice.hip lattice_plan_batch_impl: with page-locked rows a batch of >= 8192 egos is planned in K = min(E / 4096, 8) slices [E k / K, E (k + 1) / K)
SLICE_MIN_EGOS, SLICE_EGOS, SLICES_MAX = 8192, 4096, 8
# k_lattice_mixed.hip: a pipelined plan (f1p_lattice_set_pipeline) runs in at most 8 chunks of ((E + nch - 1) / nch + 3) & ~3 egos (at least 4)
PIPE_CHUNKS_MAX = 8


def compare(got, want, tol_traj=1e-9):
    """the oracle bars: nearest / best index / status bit-exact, cost 1e-10 rel, steer / speed 1e-5 (north_star), rows `tol_traj`;
    returns (max |dsteer|, max |drow|)"""
    np.testing.assert_array_equal(got["near_idx"], want["near_idx"])
    np.testing.assert_array_equal(got["best_idx"], want["best_idx"])
    np.testing.assert_array_equal(got["status"], want["status"])
    fin = np.isfinite(want["best_cost"])
    np.testing.assert_array_equal(np.isfinite(got["best_cost"]), fin)
    np.testing.assert_allclose(got["best_cost"][fin], want["best_cost"][fin], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["steer"], want["steer"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["speed"], want["speed"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["best_traj"], want["best_traj"], rtol=0, atol=tol_traj)
    return float(np.abs(got["steer"] - want["steer"]).max()), float(np.abs(got["best_traj"] - want["best_traj"]).max())


def slice_bounds(E):
    """[e_0 = 0, e_1, ..., e_K = E]: the slices of a batch with page-locked rows (K = 1: one launch)"""
    K = min(E // SLICE_EGOS, SLICES_MAX) if E >= SLICE_MIN_EGOS else 1
    return [E * k // K for k in range(K + 1)]


def chunk_bounds(E, nch):
    """[0, ce, 2 ce, ..., E]: the chunks of a plan pipelined in `nch` chunks"""
    nch = min(nch, PIPE_CHUNKS_MAX)
    ce = max(((E + nch - 1) // nch + 3) & ~3, 4)
    return list(range(0, E, ce)) + [E]


def shard_bounds(E, G):
    """[0, ..., E]: the ego ranges of a MultiContext over G contexts"""
    return [shard_range(E, g, G)[0] for g in range(G)] + [E]


def batch_cuts(E, chunks=(2, 3, 8), shards=None):
    """every place a batch of E egos is cut: slice, chunk (for each pipeline setting in `chunks`) and shard boundaries, sorted, with 0 and E"""
    cuts = set(slice_bounds(E))
    for nch in chunks:
        cuts.update(chunk_bounds(E, nch))
    if shards:
        cuts.update(shard_bounds(E, shards))
    return sorted(cuts)


def edge_egos(cuts):
    """the first and the last ego of every range between consecutive cuts"""
    out = set()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            out.update((lo, hi - 1))
    return sorted(out)
