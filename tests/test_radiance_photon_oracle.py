"""The scene list of the QA_RADIANCE_PHOTON_MAPS tests on the CPU (no GPU): oracle.photon_build fills both maps of every
(scene, sizes) pair of radiance_photon_util.SCENES, the list names every <RES, TEX, AREA> instance of the gathering kernels, and the
bake fixture with its ball made of glass fills the sizes tests/test_gpu_bake_light_photon.py uses."""
import pytest

from radiance_photon_util import INSTANCES, SCENES, case


def filled(blob, pm, cm):
    from oracle import binding as oracle
    o_pm, o_cm, emitted, emissions = oracle.photon_build(blob, oracle.photon_params(pm, cm))   # (raises when a map cannot fill)
    for table, size in ((o_pm, pm[0]), (o_cm, cm[0])):
        assert len(table) == size + 1   # (slot 0 is unused)
        for k in (1, size):
            assert table[k:k + 1].tobytes() != bytes(table.itemsize), f"record {k} of {size} is stored"
    assert all(e > 0 for e in emitted) and all(e > 0 for e in emissions)
    return emitted, emissions


@pytest.mark.parametrize("scene", list(SCENES))
def test_both_maps_fill_on_the_cpu(scene):
    blob, pm, cm, _ = case(scene)
    print(scene, pm, cm, filled(blob, pm, cm))


def test_the_scene_list_names_every_compiled_instance():
    assert {inst for _, _, inst in SCENES.values()} == INSTANCES and len(INSTANCES) == 8


def test_the_glass_ball_of_the_bake_fixture_fills_its_maps():
    from test_gpu_bake_light_photon import CAUSTICS, PHOTON, glass_ball_blob
    print(filled(glass_ball_blob(), PHOTON, CAUSTICS))
