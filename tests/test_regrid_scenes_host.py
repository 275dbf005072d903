"""Host test of what tests/test_gpu_regrid_builds.py expects and takes for granted (tests/regrid_scenes.py; no GPU): for each of
the 15 matrix scenes and each edit — move, radii, all — the oracle's frame of the edited arrays differs from the unedited one, and
r1_grid_regrid_describe of the edited arrays against the original scene's grid keeps the per-sphere invariants (every live finite sphere in
exactly one of the two lists, ids ascending in every cell, outliers ascending).  Across the matrix, by name and as inequalities: edits after
which the outlier list grows and after which it shrinks; flat axes whose one cell is re-stretched; the two scenes whose table fits the
small-scene grid kernel's LDS at the build and whose capacity does not, so that their first regrid moves them to the big form; the three
overflow inputs, one of them in the small form; and no overflow among the matrix pairs but those named in MATRIX_OVERFLOW (none).  The
rule-on adaptive call is left out where the restated rule stops every tile of the expected frame at one count: the pairs
test_update_scenes_host.ADAPTIVE_SKIP names and the product frames PRODUCT_RULE_OFF names, together at most an eighth.
Nothing here has a tolerance."""
import numpy as np
import pytest

import edge_scenes as es
import regrid_scenes as rgs
import update_scenes as us
from test_update_scenes_host import ADAPTIVE_SKIP

PAIR_IDS = [f"{c}-{k}" for c, k in rgs.PAIRS]
MATRIX_OVERFLOW = []   # the matrix pairs whose regrid overflows: none is expected; at most an eighth of the pairs, each by name
MATRIX_RULE_OFF = {("edge-inside-big", "all"), ("edge-noise_lds-big", "all"), ("leaf-n7-small", "move")}
# the product-scene frames on which the rule-on adaptive call is left out: (id, None: the original scene | the move)
#   (after `collapse` every ball stands on one point in front of the ground: every tile settles at the first count)
PRODUCT_RULE_OFF = {("large-collapse", "collapse"), ("grid40x30-collapse", "collapse")}
# the frames of the product scenes the GPU module renders: the overflow cases after the move and restored, the LDS-limit scene before and after
PRODUCT_FRAMES = [("large-collapse", "collapse"), ("large-collapse", None), ("grid40x30-collapse", "collapse"), ("grid40x30-collapse", None),
                  ("limit-under-lift", "lift"), ("limit-under-lift", None)]
SKIP_CAP = 8


def check_lists(cid, kind):
    """the per-sphere invariants of a regridded grid; returns (grid_describe, regrid_describe)"""
    built, (info, start, ids, outl) = rgs.tables(cid, kind)
    new = rgs.scene(cid, kind)[0]
    x, y, z, rsq, inv = rgs.regrid_arrays(new)
    live = np.nonzero((inv != 0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z))[0]
    assert info["spheres"] == int((inv != 0).sum()) == built[0]["spheres"]
    assert info["outliers"] == len(outl) and (np.diff(outl.astype(np.int64)) > 0).all(), (cid, kind, "outliers ascend")
    assert np.array_equal(info["cells"], built[0]["cells"]) and len(start) == len(built[1])
    if info["registrations"] == -1:
        assert not start.any() and len(ids) == 0
        assert set(outl.tolist()) <= set(live.tolist())
        return built, (info, start, ids, outl)
    assert info["registrations"] == len(ids) == int(start[-1]) and start[0] == 0 and (np.diff(start.astype(np.int64)) >= 0).all()
    assert info["registrations"] <= rgs.capacity(built)
    for q in range(len(start) - 1):
        cell = ids[start[q]:start[q + 1]].astype(np.int64)
        assert (np.diff(cell) > 0).all(), (cid, kind, "ids ascend in cell", q)
    reg, out = set(ids.tolist()), set(outl.tolist())
    assert not (reg & out) and reg | out == set(live.tolist()), (cid, kind, sorted((reg | out) ^ set(live.tolist()))[:8])
    return built, (info, start, ids, outl)


@pytest.mark.parametrize("cid,kind", rgs.PAIRS, ids=PAIR_IDS)
def test_the_edit_shows_in_the_oracles_frame_and_the_regridded_lists_hold_every_sphere_once(cid, kind):
    case = us.BY_ID[cid]
    old_rec, old_img = us.frames(case)["main"]
    new_rec, new_img = us.frames(case, kind)["main"]
    diff = int((old_img != new_img).sum())
    print(f"{cid} {kind}: {diff} bytes of the frame differ")
    assert diff > 0 and old_rec.tobytes() != new_rec.tobytes()
    for key in ("batch1", "path1"):
        assert us.frames(case, kind)[key][1].tobytes() != us.frames(case)[key][1].tobytes(), key
    built, got = check_lists(cid, kind)
    print({k: (built[0][k], got[0][k]) for k in ("registrations", "outliers")})


@pytest.mark.parametrize("cid,kind", rgs.FLIP + tuple((pid, "x") for pid in rgs.OVERFLOW_IDS), ids=lambda v: str(v))
def test_the_product_scenes_moves_show_and_their_lists_hold_every_sphere_once(cid, kind):
    if cid in rgs.PRODUCT and cid != "grid40x30-jitter":  # (`jitter` is an overflow input of this file alone: no frame of it is rendered)
        old, new = rgs.expected(cid), rgs.expected(cid, kind)
        assert old.frame0[0] != new.frame0[0] and old.records != new.records
        assert old.frames[1][0] != new.frames[1][0] and old.path1[0] != new.path1[0]
    check_lists(cid, kind)


def test_outliers_rise_and_fall_and_flat_axes_are_restretched():
    count = lambda cid, kind: tuple(t[0]["outliers"] for t in rgs.tables(cid, kind))
    rises = [p for p in rgs.PAIRS if count(*p)[1] > count(*p)[0]]
    falls = [p for p in rgs.PAIRS if count(*p)[1] < count(*p)[0]]
    print("outliers rise on", rises, "and fall on", falls)
    for pair in (("edge-palette-small", "radii"), ("edge-far-small", "all"), ("leaf-coincident-small", "move"), ("leaf-n7-small", "all")):
        assert pair in rises, pair
    for pair in (("edge-deep-big", "radii"), ("edge-deep-big", "all"), ("leaf-coincident-big", "radii")):
        assert pair in falls, pair
    # a scene that is all outliers stays one, with no registration to lose
    for kind in rgs.KINDS:
        built, got = rgs.tables("edge-far-big", kind)
        assert built[0]["registrations"] == got[0]["registrations"] == 0 and got[0]["outliers"] == got[0]["spheres"] == es.BIG_ACTIVE
    # the flat axis: one cell along y, re-stretched over the edited candidates
    stretched = []
    for cid, kind in rgs.PAIRS:
        built, got = rgs.tables(cid, kind)
        flat = np.nonzero(built[0]["cells"] == 1)[0]
        if any(built[0]["lo"][a] != got[0]["lo"][a] or built[0]["cell"][a] != got[0]["cell"][a] for a in flat):
            stretched.append((cid, kind))
        other = np.nonzero(built[0]["cells"] != 1)[0]  # "geometry kept"
        assert np.array_equal(built[0]["lo"][other], got[0]["lo"][other]) and np.array_equal(built[0]["cell"][other], got[0]["cell"][other])
    print("a flat axis is re-stretched on", stretched)
    for cid in ("root-k4-front-small", "root-wide-front-big", "edge-palette-small"):
        assert rgs.tables(cid, "move")[0][0]["cells"][1] == 1
        assert {(cid, k) for k in rgs.KINDS} <= set(stretched), cid
    # where nothing but the stretch can show, the id tables are the build's
    for cid, kind in (("root-k4-front-small", "move"), ("root-k4-front-small", "radii"), ("root-wide-front-big", "move"), ("root-wide-front-big", "radii")):
        built, got = rgs.tables(cid, kind)
        assert built[2].tobytes() == got[2].tobytes() and built[1].tobytes() == got[1].tobytes()
    # and everywhere else the tables change: all but a few pairs
    same = [p for p in rgs.PAIRS if rgs.tables(*p)[0][2].tobytes() == rgs.tables(*p)[1][2].tobytes()]
    assert len(same) * 4 <= len(rgs.PAIRS), same


@pytest.mark.parametrize("cid,kind", rgs.FLIP, ids=lambda v: str(v))
def test_the_first_regrid_moves_the_scene_to_the_big_form(cid, kind):
    """r1_scene_grid.cpp: the build keeps the small form while n_start + registrations <= R1_GRID_LDS_HALVES; regrid_layout while
    n_start + capacity does.  launch_info does not show which form runs: this is the evidence."""
    built, got = rgs.tables(cid, kind)
    n_start = len(built[1])
    assert built[0]["spheres"] <= 1023 and built[0]["registrations"] < 65536
    assert n_start + built[0]["registrations"] <= rgs.LDS_HALVES < n_start + rgs.capacity(built)
    assert 0 < got[0]["registrations"] <= rgs.capacity(built)  # no overflow: the big form walks the grid


def test_the_overflow_inputs_overflow_and_no_matrix_pair_does():
    for cid in rgs.OVERFLOW_IDS:
        built, got = rgs.tables(cid, "x")
        assert got[0]["registrations"] == -1 and not got[1].any() and len(got[2]) == 0, cid
    built = rgs.tables("large-collapse", "x")[0]
    assert built[0]["spheres"] <= 1023 and len(built[1]) + rgs.capacity(built) <= rgs.LDS_HALVES  # the small form, before and after
    assert rgs.tables("grid40x30-collapse", "x")[0][0]["spheres"] > 1023                           # the big form
    over = [p for p in rgs.PAIRS if rgs.tables(*p)[1][0]["registrations"] == -1]
    assert over == MATRIX_OVERFLOW and len(MATRIX_OVERFLOW) * SKIP_CAP <= len(rgs.PAIRS), over


def test_the_rule_on_adaptive_call_is_left_out_on_the_named_frames_alone():
    off = {p for p in rgs.PAIRS if p in ADAPTIVE_SKIP}
    assert off == MATRIX_RULE_OFF, off
    for pair in rgs.PAIRS:
        assert rgs.rule_shows(us.expected(*pair)) == (pair not in ADAPTIVE_SKIP), pair
    product_off = {(cid, kind) for cid, kind in PRODUCT_FRAMES if not rgs.rule_shows(rgs.expected(cid, kind))}
    print("the rule stops every tile at one count on", sorted(off), "and", product_off)
    assert product_off == PRODUCT_RULE_OFF, product_off
    assert (len(off) + len(product_off)) * SKIP_CAP <= len(rgs.PAIRS) + len(PRODUCT_FRAMES)


def test_the_rounds_and_the_dropped_sphere_show():
    for cid in rgs.ROUND_IDS:
        frames = [rgs.round_expected(cid, seed).frame0[0] for seed in rgs.ROUND_SEEDS] + [us.expected(cid).frame0[0]]
        assert len(set(frames)) == len(frames), (cid, "every round's frame differs from the others and from the original")
        for seed in rgs.ROUND_SEEDS:
            new = rgs.round_scene(cid, seed)
            assert (new.arrays["inv_radius"] != 0).tolist() == (us.scene(cid)[0].arrays["inv_radius"] != 0).tolist()
    assert rgs.round_scene(rgs.ROUND_IDS[0], 41).arrays["center_x"].tobytes() == us.scene(rgs.ROUND_IDS[0], "all")[0].arrays["center_x"].tobytes()
    for cid in rgs.DEVICE_IDS:
        sphere = rgs.dropped_sphere(cid)
        sa, _ = us.scene(cid)
        assert sa.arrays["inv_radius"][sphere] != 0
        assert rgs.dropped_expected(cid).frame0[0] != us.expected(cid).frame0[0], (cid, sphere, "the sphere that goes must show in the frame")
