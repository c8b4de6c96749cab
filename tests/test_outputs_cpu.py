"""lwsnet_amd/outputs.py on the host: merge_keep, the one statement of the rule for the code map that the geometry and photometric
outputs are given, on all eight combinations of its three maps against the rule written out in numpy."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

# [1,1,2,3] and [1,1,2,4]: every code 0 / 1 / 2 / 3 of `keep` meets a 0 and a 1 of each mask, and each mask's 0 meets the other's 0 and 1
KEEP = np.array([0, 1, 2, 3] * 4, np.uint8).reshape(1, 1, 2, 8)
VALID_LEFT = np.array([0] * 4 + [1] * 4 + [0] * 4 + [1] * 4, np.uint8).reshape(1, 1, 2, 8)
CONF_LOW = np.array([0] * 8 + [1] * 8, np.uint8).reshape(1, 1, 2, 8)


def rule(keep, valid_left, conf_low):
    """conf_low first: where it is 0 the code becomes 0, or it is the map itself when there is none; valid_left next: where it is 0
    the code becomes 2, or it is the map itself."""
    if conf_low is not None:
        keep = conf_low.copy() if keep is None else np.where(conf_low == 0, 0, keep).astype(np.uint8)
    if valid_left is not None:
        keep = valid_left.copy() if keep is None else np.where(valid_left == 0, 2, keep).astype(np.uint8)
    return keep


@pytest.mark.parametrize("shape", [(1, 1, 2, 3), (1, 1, 2, 8)])
@pytest.mark.parametrize("has_keep,has_valid,has_conf", list(itertools.product([False, True], repeat=3)))
def test_merge_keep(has_keep, has_valid, has_conf, shape):
    from lwsnet_amd.outputs import merge_keep
    if shape == (1, 1, 2, 3):       # codes 0 1 2 / 3 0 1 under masks that put a 0 and a 1 over each row
        maps = (np.array([[0, 1, 2], [3, 0, 1]], np.uint8), np.array([[0, 1, 0], [1, 0, 1]], np.uint8), np.array([[1, 0, 0], [0, 1, 1]], np.uint8))
        maps = [m.reshape(shape) for m in maps]
    else:
        maps = [KEEP, VALID_LEFT, CONF_LOW]
    keep, valid_left, conf_low = (m if on else None for m, on in zip(maps, (has_keep, has_valid, has_conf)))
    before = [None if m is None else m.copy() for m in (keep, valid_left, conf_low)]
    t = [None if m is None else torch.from_numpy(m) for m in (keep, valid_left, conf_low)]
    got = merge_keep(t[0], valid_left=t[1], conf_low=t[2])
    want = rule(keep, valid_left, conf_low)
    if want is None:
        assert got is None
    else:
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape
        assert np.array_equal(got.numpy(), want)
    for m, b in zip((keep, valid_left, conf_low), before):
        assert m is None or np.array_equal(m, b), "the inputs are left as they were"


def test_merge_keep_table_covers_every_code_under_every_mask_value():
    for mask in (VALID_LEFT, CONF_LOW):
        assert {(int(k), int(m)) for k, m in zip(KEEP.ravel(), mask.ravel())} == set(itertools.product(range(4), range(2)))
    assert rule(KEEP, VALID_LEFT, CONF_LOW).ravel().tolist() == [2, 2, 2, 2, 0, 0, 0, 0, 2, 2, 2, 2, 0, 1, 2, 3]


def test_geometry_table_names_every_geometry_flag():
    """_geometry_requested is derived from the table the geometry writer iterates: each flag alone asks for it, no other flag does."""
    from lwsnet_amd import inference, outputs
    flags = [flag for flags, _ in outputs.GEOMETRY for flag in flags]
    assert flags == ["save_disp16", "save_depth", "save_ply", "save_normals", "save_mesh", "ground", "save_ground", "stixels", "save_stixels"]
    assert inference._geometry_requested is outputs.geometry_requested
    p = inference.build_parser()
    assert not inference._geometry_requested(p.parse_args(["--save_conf", "--photometric", "--save_photo", "--lr_check", "1", "--save_rect"]))
    for flag in flags:
        assert inference._geometry_requested(p.parse_args(["--" + flag])), flag


def test_default_arguments_are_the_checks_defaults():
    """A namespace that skipped main()'s checks is given what they would have written, in their order."""
    from lwsnet_amd import inference
    p = inference.build_parser()
    checked, plain = p.parse_args([]), p.parse_args([])
    for check in (inference.check_lr_arguments, inference.check_occ_arguments, inference.check_speckle_arguments, inference.check_wmedian_arguments,
                  inference.check_geometry_arguments, inference.check_rectify_arguments, inference.check_conf_arguments):
        check(p, checked)
    inference.post.check_photometric_arguments(p, checked, save=True)
    inference.default_arguments(plain)
    assert list(vars(plain).items()) == list(vars(checked).items())
    assert (plain.sigma_max, plain.photo_alpha, plain.max_jump, plain.stixel_width, plain.ground_tol) == (8.0, 0.85, 1.0, 8, 0.2)
    implied = p.parse_args(["--save_stixels"])
    inference.default_arguments(implied)
    assert implied.stixels and implied.ground and not implied.save_ground
