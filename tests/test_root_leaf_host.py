"""Host test of the scenes tests/test_gpu_root_leaf.py renders (tests/root_leaf_scenes.py): every scene's tree has the root
leaf its name promises — pair count, the spheres of its slots, the flat axis — in both table orders and both sizes, and the oracle's frame of
`twins` shows which of the two coincident balls won the ties."""
import numpy as np
import pytest

import edge_scenes as es
import root_leaf_scenes as rs


@pytest.mark.parametrize("size", rs.SIZES)
@pytest.mark.parametrize("order", rs.ORDERS)
@pytest.mark.parametrize("name", rs.SCENES)
def test_the_scenes_have_the_root_leaves_the_gpu_test_is_about(name, order, size):
    rs.assert_shape(name, order, size)


@pytest.mark.parametrize("order", rs.ORDERS)
def test_the_wide_lattice_gives_the_big_scene_kernels_a_root_leaf_of_two_full_pairs(order):
    rs.assert_shape(rs.WIDE, order, "big")
    assert es.active(rs.build(rs.WIDE, order, "big")[0]) > 1023


def test_the_shapes_cover_what_the_root_step_can_meet():
    shapes = {(p, tuple(k >= 0 for k in slots)) for p, slots, _ in rs.SHAPE.values()}
    assert shapes == {(1, (True, False)), (1, (True, True)), (2, (True, True, True, False)), (2, (True, True, True, True))}
    assert not rs.SHAPE["k5"][2] and all(flat for name, (_, _, flat) in rs.SHAPE.items() if name != "k5")
    a, b = rs.OUTLIERS["twins"][1:3]
    assert a == b  # same centre, same radius
    assert all(c[2] < rs.CAMERA_FROM[2] - 1.0 - r for c, r in rs.OUTLIERS["behind"])  # wholly behind the camera


@pytest.mark.parametrize("order", rs.ORDERS)
def test_a_wrong_tie_between_the_twins_shows_in_the_frame(order):
    """The twins differ in material alone; with the materials swapped the oracle's frame changes, so a kernel that gave the ties to the
    higher index would render other pixels."""
    sa, _ = rs.build("twins", order, "small")
    a, b = rs.outlier_ids("twins", order)[1:3]
    assert any(sa.arrays[k][a] != sa.arrays[k][b] for k in ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param"))
    img, rays, rec = rs.oracle("twins", order, "small", "frame")
    simg, srays, srec = rs.oracle("twins", order, "small", "swapped")
    differ = int((np.frombuffer(img, np.uint8) != np.frombuffer(simg, np.uint8)).sum())
    print("bytes that differ between the twins' two frames:", differ)
    assert differ > 100
