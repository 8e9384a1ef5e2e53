"""Layout of an MSM partial-sum buffer (csrc/msm_part_layout.h): chunk partials, group sums, window
sums, and for comb tables the common sums, the counts, lane 0's digits of the uniform groups and
the list of those groups -- everything the tail of an MSM reads, possibly on another stream than
the one that already prepares the next MSM.  tests/native/msm_part_layout_check.cpp prints the
regions through the function msm_impl.h uses; built plain and with -fsanitize=address,undefined,
the two builds must print the same.  Order, disjointness and alignment are checked here."""
import itertools

import pytest

from tests import native_build

pytestmark = native_build.needs_gxx
REGIONS = ["partial", "mid", "wsum", "usum", "counts", "d0", "ulist"]
ELEMS = (128, 256)                  # one G1 / G2 accumulator
CHUNKS = (1, 16)
NGROUPS = (1, 4)
WINDOWS = (254, 255)
BPS = (64, 1024)
GROUPS = (1, 10, 3450)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return native_build.build("msm_part_layout_check.cpp", tmp_path_factory.mktemp("msm_part_layout"))


def _layouts(exes, configs):
    args = [str(x) for c in configs for x in c]
    _, out, _ = native_build.run_both(exes, args)
    res = {}
    for line in out.splitlines():
        f = line.split()
        cfg = tuple(int(x) for x in f[:7])
        entry = res.setdefault(cfg, {"regions": [], "bytes": None})
        if f[7] == "bytes":
            entry["bytes"] = int(f[8])
        else:
            entry["regions"].append((f[7], int(f[8]), int(f[9]), int(f[10])))
    assert set(res) == set(configs)
    return res


def _check(cfg, lay):
    elem, chunks, ngroups, W, Bp, G, common = cfg
    regs = lay["regions"]
    assert [r[0] for r in regs] == REGIONS
    want = {"partial": chunks * W * Bp * elem, "mid": ngroups * W * Bp * elem, "wsum": W * Bp * elem,
            "usum": W * elem * common, "counts": 8 * common, "d0": W * G * 4 * common,
            "ulist": G * 4 * common}
    end = 0
    for name, off, size, align in regs:
        assert size == want[name], (cfg, name)
        assert off >= end, (cfg, name, "overlaps the region before it")    # disjoint and in order
        assert off == end, (cfg, name, "leaves a hole")
        assert align == (elem if name in ("partial", "mid", "wsum", "usum") else 4)
        assert off % align == 0 and size % align == 0, (cfg, name)
        end = off + size
    assert lay["bytes"] == end


@pytest.mark.parametrize("elem", ELEMS)
def test_regions_are_disjoint_ordered_and_aligned(exes, elem):
    configs = [(elem, c, g, w, bp, G, 1)
               for c, g, w, bp, G in itertools.product(CHUNKS, NGROUPS, WINDOWS, BPS, GROUPS)]
    assert len(configs) == 48
    res = _layouts(exes, configs)
    for cfg in configs:
        _check(cfg, res[cfg])


def test_shared_table_layout_has_no_comb_regions(exes):
    configs = [(elem, c, g, 17, bp, 0, 0)
               for elem, c, g, bp in itertools.product(ELEMS, CHUNKS, NGROUPS, BPS)]
    res = _layouts(exes, configs)
    for cfg in configs:
        _check(cfg, res[cfg])
        assert res[cfg]["bytes"] == (cfg[1] + cfg[2] + 1) * 17 * cfg[4] * cfg[0]


def test_headline_sizes(exes):
    # Arbo-160, batch 1024: the largest d0 is the [255][3450] of the issue's bound, 3.5 MB
    cfg = (128, 16, 4, 255, 1024, 3450, 1)
    lay = _layouts(exes, [cfg])[cfg]
    sizes = {r[0]: r[2] for r in lay["regions"]}
    assert sizes["d0"] == 255 * 3450 * 4 <= 3.6e6
    assert sizes["ulist"] == 3450 * 4
