"""A long-lived Context's results do not depend on its history: every session of tests/session_script.py is played on one Context, and
each query is repeated on a fresh witness Context that is given only the current values of the mutators the query reads (in one canonical
order) and, for the stateful planners, the data the long-lived context carries -- its warm starts through *_warm_get / *_warm_set, its
closed-loop headings as an explicit prev_theta.  Every returned array must be equal bit for bit (NaNs included), dtype and shape too; where
the session expects an error, both contexts must raise the same one.  There is no tolerance and no exemption (session_script.EXEMPT is
empty).

A lattice_step of a running chain has no witness form of its own (a fresh context has no chain): the witness runs lattice_plan with the
chain's headings as prev_theta, and steer, speed, status and the kept rows must equal the step's.

A failure names the seed, the operation's index and kind, and the last mutator of each kind before it; session_script.replay with the
same seed on a host-side driver, or a cut of script(seed), reproduces the sequence offline.  The test does not retry or bisect.

Measured on an MI355X (one process, this module alone): 2.4 s for the first seed -- it loads the library and pays every
kernel's first launch -- and 1.6 s for each of the others; 319 queries and so 319 witnesses per seed.  The witnesses are most of it:
1.2 s per seed, 3.7 ms each for creating the Context, giving it what the query reads and closing it.  A bare Context(0) ... close() is
2.75 ms (median of 30); with a 320-point raceline, three tracks and a 170 x 150 grid it is 3.23 ms.  The test prints these figures (-s).

Whether the comparison can fail is shown on the CPU (tests/test_session_script_host.py: a fake context that keeps a stale grid is
reported at the right operation).  The schedule switches (lattice mode, clearance, pipeline, split, order, pursuit form, kmpc / stmpc mode,
groups, QP pack) are documented to leave the outputs bit-identical, so for them the test pins that claim across the whole session.
"""
import time

import pytest

import session_script as ss

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_results_do_not_depend_on_the_contexts_history(seed):
    ops = ss.script(seed)
    stats = {}
    t0 = time.perf_counter()
    try:
        ss.replay(ops, ss.Driver(), seed=seed, stats=stats)
    finally:
        if stats:
            print(f"seed {seed}: {time.perf_counter() - t0:.2f} s, {stats['queries']} queries, witnesses {stats['witness_seconds']:.2f} s "
                  f"({1e3 * stats['witness_seconds'] / max(stats['queries'], 1):.1f} ms each)")
