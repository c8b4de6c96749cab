"""The plan matrix of tests/test_gpu_plan_matrix.py, checked on the CPU: its launch-count model reproduces the counts the
profiler test pins, every shape is legal, and every host predicate of lws_forward keeps cells on both sides, one per cause --
the conditions that keep the matrix from silently shrinking."""
import plan_matrix as pm
from lwsnet_amd.weights import default_args


def test_module_is_pure_python():
    """plan_matrix restates host logic; it must be importable where neither torch nor the library is."""
    import ast
    with open(pm.__file__) as f:
        tree = ast.parse(f.read())
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]


def test_model_reproduces_the_pinned_counts():
    """tests/test_gpu_parity.py::test_profiler_counts_and_sampling: 41 launches of the default plan at batch 1, 64x256; 42 with
    refinement1_left's first convolution as its own launch."""
    e = pm.expected_launches({}, default_args(), 1, 64, 256)
    assert e["total"] == 41 and e["ref_first"] == 0 and e["ref_dws"] == 11 and e["upsample_add"] == 0 and e["softargmin"] == 0
    assert e["conv3d_mid16"] == 4 and e["conv3d_mid8"] == 8 and e["conv3d_last"] == 3 and e["volume_l1_shift+conv3d_first"] == 3
    assert e["volume_l1_warp"] == 2 and e["ref_conv64"] == 1 and e["ref_last"] == 1 and e["feature_conv2d"] == 8
    assert e["defers"] == [True, True, True] and e["integer_ratio"] == [True, True, True] and e["fuse_ref_last"] is True
    assert e["nchunks"] == 1 and e["pipe"] is False
    e = pm.expected_launches({"fuse_first": 1}, default_args(), 1, 64, 256)
    assert e["total"] == 42 and e["ref_first"] == 1 and e["ref_dws"] == 11


def test_model_by_hand_at_the_other_sides():
    """Cells worked out by hand from lws_forward.hip, one per branch of stage_map and of the refinement."""
    a = default_args()
    # batch 3 at an even size: nothing deferred, stage 1 unfused -> k_softargmin_upsample, stages 2, 3 fused -> k_upsample_add
    e = pm.expected_launches({}, a, 3, 64, 256)
    assert e["defers"] == [False] * 3 and e["fused"] == [False, True, True] and e["softargmin"] == 1 and e["upsample_add"] == 2
    assert e["ref_dws"] == 12 and e["ref_last"] == 1 and e["fuse_ref_last"] is False and e["total"] == 45
    # an odd size: the ratio is no integer, stage 1 is k_softargmin + k_upsample_add
    e = pm.expected_launches({}, a, 1, 63, 255)
    assert e["integer_ratio"] == [False] * 3 and e["softargmin"] == 1 and e["upsample_add"] == 3 and e["ref_dws"] == 11
    # stage 1 not fused at batch 1, stages 2 and 3 still deferred
    e = pm.expected_launches({"fuse_last1": 0}, a, 1, 64, 256)
    assert e["defers"] == [False, True, True] and e["softargmin"] == 1 and e["upsample_add"] == 0 and e["total"] == 42
    # refinement1_disp's first convolution as its own launch: stage 3's map cannot wait for it
    e = pm.expected_launches({"fuse_first": 2}, a, 1, 64, 256)
    assert e["defers"] == [True, True, False] and e["upsample_add"] == 1 and e["ref_first"] == 1 and e["total"] == 43
    # one pair per chunk at batch 5: five chunks on both refinement branches, the pipe on automatically
    e = pm.expected_launches({"ref_chunk_mb": 1}, a, 5, 64, 256)
    assert e["CH"] == 1 and e["nchunks"] == 5 and e["pipe"] is True and e["ref_dws"] == 5 * 12 and e["ref_conv64"] == 5
    # the issue's ragged cell: 15x191 with 1 MB chunks is two pairs per chunk; batch 8 is four chunks
    e = pm.expected_launches({"ref_chunk_mb": 1}, a, 3, 15, 191)
    assert e["CH"] == 2 and e["nchunks"] == 2 and e["ragged"] and not e["pipe"]
    e = pm.expected_launches({"ref_chunk_mb": 1}, a, 8, 15, 191)
    assert e["CH"] == 2 and e["nchunks"] == 4 and not e["ragged"] and e["pipe"]
    # lws_forward_conf: nothing deferred or fused, one k_softargmin_conf per stage
    e = pm.expected_launches({}, a, 1, 64, 256, conf=True)
    assert e["defers"] == [False] * 3 and e["fused"] == [False] * 3 and e["softargmin"] == 3 and e["softargmin_conf"] == 3


def test_matrix_is_what_the_gpu_tests_walk():
    assert pm.PLANS[:20] == pm.OPTION_PLANS and len(pm.PLANS) == 29 and {} in pm.PLANS
    assert len({pm.plan_id(p) for p in pm.PLANS}) == len(pm.PLANS)
    assert all(set(p) <= set(pm.OPTION_DEFAULTS) for p in pm.PLANS)
    assert sorted(pm.WALK) == sorted(pm.SHAPES) and all(pm.size_ok(H, W) for H, W in pm.SHAPES)
    assert not pm.size_ok(30, 256) and not pm.size_ok(8, 184)
    for shape in pm.SHAPES:
        assert pm.BATCHES[shape][:3] == (1, 2, 3)
        assert (5 in pm.BATCHES[shape]) == (shape not in pm.LARGE_SHAPES)
    assert 8 in pm.BATCHES[(15, 191)]
    assert sum(1 for _ in pm.cells()) == len(pm.PLANS) * sum(len(b) for b in pm.BATCHES.values())


def test_every_predicate_has_cells_on_both_sides():
    cov = pm.coverage(pm.PLANS, pm.SHAPES, pm.BATCHES, default_args())
    empty = [k for k, v in cov.items() if not v]
    assert not empty, f"no cell of the matrix reaches: {empty}"
    # the cells the issue names
    assert ("ref_chunk_mb=1", (15, 191), 8) in cov["pipe:on automatically"]
    assert ("ref_chunk_mb=1", (15, 191), 3) in cov["nchunks:ragged last chunk"]
    assert ("fuse_ref_last=1,ref_chunk_mb=1", (15, 191), 3) in cov["nchunks:ragged last chunk"]        # k_ref_dws_last on it
    assert ("side_streams=0,ref_pipe=1,ref_chunk_mb=1", (15, 191), 8) in cov["pipe:refused by side_streams=0"]
    assert ("ref_pipe=1,ref_chunk_mb=1", (15, 191), 3) in cov["pipe:refused by 2*CH>B"]
    assert ("warp_form=0", (24, 200), 2) in cov["defers:on at B=2"]                  # a DeferredMap in the gather form, partial tiles
    assert ("default", (63, 255), 2) in cov["integer_ratio:no"]
