"""The tail of a comb MSM (csrc/msm_impl.h: comb_eff_chunks, msm_accumulate_comb, msm_reduce).

Only the groups whose scalars vary across the batch go through the per-lane accumulate kernel, and
the number of chunks they are split into -- hence the number of partial sums the reduction reads --
follows their count: one chunk per M = zkmi_comb_min_groups_per_chunk() varying groups, at least
one, at most the chunks of the launch grid.  The partials are packed accumulators of the 29-bit
field form and are summed with ec29.h's padd29.  These tests put the number of varying groups on
both sides of every chunk boundary (0, 1, M, M + 1, 2M and all 2M + 1 groups), at the end of the
base list and spread over it, and compare every real lane with the C oracle.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_fullsize import _rand_fr_array

pytestmark = pytest.mark.gpu

K = 6
LAYOUTS = ("end", "spread")


@functools.lru_cache(maxsize=None)
def _shape(m):
    """(groups, bases): 2M + 1 groups of 6, the last one ragged (4 bases)"""
    g = 2 * m + 1
    return g, K * g - 2


@pytest.fixture(scope="module")
def tail(zk_ctx):
    """The bases (random multiples of the generator), their comb tables, the scalar vectors and the
    oracle's results, each made once and shared by the cases."""
    m = zk_ctx.comb_min_groups_per_chunk()
    assert m >= 1
    G, N = _shape(m)

    class Tail:
        M = m
        bases, handles, vectors, wants = {}, {}, {}, {}

        def get_bases(self, group):
            if group not in self.bases:
                rng = np.random.default_rng(90 + group)
                gen = H.g1_gen_mont() if group == 1 else H.g2_gen_mont()
                out = np.zeros((N, 8 if group == 1 else 16), dtype=np.uint64)
                zk_ctx.fixed_base_mul(group, gen, _rand_fr_array(rng, (N,)), N, out)
                self.bases[group] = out
            return self.bases[group]

        def handle(self, group, wb):
            if (group, wb) not in self.handles:
                self.handles[group, wb] = zk_ctx.msm_bases_load(group, self.get_bases(group), N, wb)
            return self.handles[group, wb]

        def scalars(self, nv, layout):
            """three scalar vectors [3][N] that agree outside the nv varying groups and differ in
            every scalar of those"""
            if (nv, layout) not in self.vectors:
                rng = np.random.default_rng(7000 + 10 * nv + LAYOUTS.index(layout))
                if layout == "end":
                    var = list(range(G - nv, G))
                else:   # nv groups spread evenly over all of them
                    var = [g for g in range(G) if (g * nv) // G != ((g + 1) * nv) // G]
                assert len(var) == nv
                vec = np.broadcast_to(_rand_fr_array(rng, (N,)), (3, N, 4)).copy()
                for g in var:
                    sl = slice(g * K, min((g + 1) * K, N))
                    vec[:, sl] = _rand_fr_array(rng, (3, len(range(N)[sl])))
                self.vectors[nv, layout] = vec
            return self.vectors[nv, layout]

        def want(self, group, nv, layout, i):
            from oracle import cref
            key = (group, nv, layout, i)
            if key not in self.wants:
                self.wants[key] = cref.msm(group, self.get_bases(group), self.scalars(nv, layout)[i])
            return self.wants[key]

        def check(self, group, wb, batch, nv, layout):
            vec = self.scalars(nv, layout)
            lanes = np.arange(batch) % 3          # lanes 0 and 1 always differ where groups vary
            sc = np.ascontiguousarray(vec[lanes])
            res = np.zeros((batch, self.get_bases(group).shape[1]), dtype=np.uint64)
            zk_ctx.msm_batch(self.handle(group, wb), sc, batch, res)
            for p in range(batch):
                assert np.array_equal(res[p], self.want(group, nv, layout, int(lanes[p]))), \
                    (group, wb, batch, nv, layout, p)

    t = Tail()
    yield t
    for h in t.handles.values():
        zk_ctx.msm_bases_free(h)


# number of varying groups in units of (M, 1): 0, 1, M, M + 1, 2M, 2M + 1 = all
COUNTS = {"0": (0, 0), "1": (0, 1), "M": (1, 0), "M+1": (1, 1), "2M": (2, 0), "all": (2, 1)}
CASES = [(c, layout) for c in COUNTS for layout in LAYOUTS
         if not (c in ("0", "all") and layout == "spread")]   # nothing to place differently


@pytest.mark.parametrize("count,layout", CASES, ids=[f"{c}-{layout}" for c, layout in CASES])
@pytest.mark.parametrize("batch", [2, 65])
@pytest.mark.parametrize("wb", [200 + K, 300 + K])
@pytest.mark.parametrize("group", [1, 2])
def test_msm_comb_tail_vs_oracle(tail, group, wb, batch, count, layout):
    a, b = COUNTS[count]
    tail.check(group, wb, batch, a * tail.M + b, layout)


@pytest.mark.parametrize("wb", [200 + K, 300 + K])
@pytest.mark.parametrize("group", [1, 2])
def test_msm_comb_tail_skips_stale_partials(tail, group, wb):
    """Every group varies, then only one, on the same handle: the second launch writes one chunk
    partial, and the slots beside it still hold the first batch's."""
    G, _ = _shape(tail.M)
    tail.check(group, wb, 65, G, "end")
    tail.check(group, wb, 65, 1, "end")
    tail.check(group, wb, 65, 0, "end")
