"""GPU test of the ray queries (r1_query_kernels.hip) over the scenes of tests/edge_scenes.py, small and big: 4096 rays per scene — the frame's
primary rays, scatter rays from their hit points and a sixteenth with t_max at the hit's own t and at its two fp32 neighbours
(edge_scenes.cast_rays) — CLOSEST and ANY through the box tree, the uniform grid and the reference form.  Every answer must equal
r1_cast_rays_host's (every ray against every sphere, pinned to the reference by tests/test_cast_host.py), byte for byte."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
from test_gpu_cast import same_hits

pytestmark = pytest.mark.gpu

VARIANTS = {"tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "reference": binding.VARIANT_REFERENCE}


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("size", es.SIZES)
@pytest.mark.parametrize("name", es.SCENES)
def test_casts_equal_the_host_form(renderer, name, size):
    sa, _ = es.build(name, size)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    rays = es.cast_rays(name, size)
    want = binding.cast_rays_host(es.cscene(sa), rays)
    frac = float((want["index"] >= 0).mean())
    print(name, size, "hit fraction", frac)
    assert 0.2 <= frac <= 0.8, frac
    want_any = (want["index"] >= 0).astype(np.uint8)
    assert binding.cast_rays_host(es.cscene(sa), rays, binding.CAST_ANY).tobytes() == want_any.tobytes()
    for tag, variant in VARIANTS.items():
        same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, variant), want, (name, size, tag))
        same_hits(renderer.cast_rays(rays, binding.CAST_ANY, variant), want_any, (name, size, tag, "any"))
