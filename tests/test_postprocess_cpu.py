"""The rules of the post-processing chain (lwsnet_amd/postprocess.py) without a GPU: the facts Options derives from the stage
switches against a table written out by hand, two restatements of what the CLIs computed before the chain had one home, and the
range errors of Options.check."""
import itertools

import pytest

import test_speckle_cpu
import test_wmedian_cpu
from lwsnet_amd import evaluate, inference
from lwsnet_amd.postprocess import Options

FACTS = ("forward_fills", "speckle_fills", "row_filled", "filled", "needs_guide", "wmedian_takes_codes", "geometry_takes_codes")

# (left-right check, speckle filter, weighted median, sigma) -> FACTS in their order, T = true.  The switches: "off", "on", and on
# with the stage's fill ("fill": --lr_fill / --speckle_fill; "fill0" / "fill4": --wmedian_fill 0 / 4).  The specification, by hand:
# the forward fills only without a speckle filter behind it; the speckle filter fills for either row-fill flag; the guide goes
# with the median and sigma > 0; the median takes codes when a step before it made some and no row was filled; the geometry files
# take them when, in addition, the median filled no hole.
TABLE = {
    ('off',   'off',   'off',     0): ".......",
    ('off',   'off',   'off',    10): ".......",
    ('off',   'off',   'fill0',   0): ".......",
    ('off',   'off',   'fill0',  10): "....T..",
    ('off',   'off',   'fill4',   0): "...T...",
    ('off',   'off',   'fill4',  10): "...TT..",
    ('off',   'on',    'off',     0): "......T",
    ('off',   'on',    'off',    10): "......T",
    ('off',   'on',    'fill0',   0): ".....TT",
    ('off',   'on',    'fill0',  10): "....TTT",
    ('off',   'on',    'fill4',   0): "...T.T.",
    ('off',   'on',    'fill4',  10): "...TTT.",
    ('off',   'fill',  'off',     0): ".TTT...",
    ('off',   'fill',  'off',    10): ".TTT...",
    ('off',   'fill',  'fill0',   0): ".TTT...",
    ('off',   'fill',  'fill0',  10): ".TTTT..",
    ('off',   'fill',  'fill4',   0): ".TTT...",
    ('off',   'fill',  'fill4',  10): ".TTTT..",
    ('on',    'off',   'off',     0): "......T",
    ('on',    'off',   'off',    10): "......T",
    ('on',    'off',   'fill0',   0): ".....TT",
    ('on',    'off',   'fill0',  10): "....TTT",
    ('on',    'off',   'fill4',   0): "...T.T.",
    ('on',    'off',   'fill4',  10): "...TTT.",
    ('on',    'on',    'off',     0): "......T",
    ('on',    'on',    'off',    10): "......T",
    ('on',    'on',    'fill0',   0): ".....TT",
    ('on',    'on',    'fill0',  10): "....TTT",
    ('on',    'on',    'fill4',   0): "...T.T.",
    ('on',    'on',    'fill4',  10): "...TTT.",
    ('on',    'fill',  'off',     0): ".TTT...",
    ('on',    'fill',  'off',    10): ".TTT...",
    ('on',    'fill',  'fill0',   0): ".TTT...",
    ('on',    'fill',  'fill0',  10): ".TTTT..",
    ('on',    'fill',  'fill4',   0): ".TTT...",
    ('on',    'fill',  'fill4',  10): ".TTTT..",
    ('fill',  'off',   'off',     0): "T.TT...",
    ('fill',  'off',   'off',    10): "T.TT...",
    ('fill',  'off',   'fill0',   0): "T.TT...",
    ('fill',  'off',   'fill0',  10): "T.TTT..",
    ('fill',  'off',   'fill4',   0): "T.TT...",
    ('fill',  'off',   'fill4',  10): "T.TTT..",
    ('fill',  'on',    'off',     0): ".TTT...",
    ('fill',  'on',    'off',    10): ".TTT...",
    ('fill',  'on',    'fill0',   0): ".TTT...",
    ('fill',  'on',    'fill0',  10): ".TTTT..",
    ('fill',  'on',    'fill4',   0): ".TTT...",
    ('fill',  'on',    'fill4',  10): ".TTTT..",
    ('fill',  'fill',  'off',     0): ".TTT...",
    ('fill',  'fill',  'off',    10): ".TTT...",
    ('fill',  'fill',  'fill0',   0): ".TTT...",
    ('fill',  'fill',  'fill0',  10): ".TTTT..",
    ('fill',  'fill',  'fill4',   0): ".TTT...",
    ('fill',  'fill',  'fill4',  10): ".TTTT..",
}


def flags(lr, sp, wm, sigma):
    """The switches of a TABLE key as the flags of the CLIs."""
    return dict(lr_check=None if lr == "off" else 1.0, lr_fill=lr == "fill", speckle=None if sp == "off" else 60, speckle_diff=1.0,
                speckle_fill=sp == "fill", wmedian=None if wm == "off" else 2, wmedian_sigma=float(sigma),
                wmedian_fill=4 if wm == "fill4" else 0)


def former_inference(lr_check, lr_fill, speckle, speckle_diff, speckle_fill, wmedian, wmedian_sigma, wmedian_fill):
    """FACTS as inference.inference computed them while it ran the chain itself (its expressions, names kept)."""
    lr, sp, wm = lr_check is not None, speckle is not None, wmedian is not None
    row_filled = lr_fill or (sp and speckle_fill)
    filled = row_filled or (wm and wmedian_fill > 0)
    forward_fill = lr and (lr_fill and not sp)                          # forward_lr(fill=args.lr_fill and not sp)
    speckle_fill_ = sp and row_filled                                   # speckle_stages(..., row_filled)
    guide = wm and wmedian_sigma > 0
    keep = sp or lr                                                     # keep = sp_masks if sp else lr_masks
    median_codes = wm and keep and not row_filled                       # None if row_filled else keep
    geometry_codes = keep and not filled                                # masks[stage] if masks is not None and not filled else None
    return dict(zip(FACTS, map(bool, (forward_fill, speckle_fill_, row_filled, filled, guide, median_codes, geometry_codes))))


def former_evaluate(lr_check, lr_fill, speckle, speckle_diff, speckle_fill, wmedian, wmedian_sigma, wmedian_fill):
    """The FACTS that evaluate.evaluate and its _sequential computed (their expressions, names kept); it writes no geometry file."""
    lr = None if lr_check is None else (float(lr_check), bool(lr_fill))
    sp = None if speckle is None else (int(speckle), float(speckle_diff), bool(speckle_fill or lr_fill))
    wm = None if wmedian is None else (int(wmedian), float(wmedian_sigma), int(wmedian_fill))
    if sp is not None and lr is not None:
        lr = (lr[0], False)
    row_filled = (lr is not None and lr[1]) or (sp is not None and sp[2])
    keep = sp is not None or lr is not None                             # sp_masks if sp is not None else (None if lr is None else res.mask)
    facts = {"forward_fills": lr is not None and lr[1], "speckle_fills": sp is not None and sp[2], "row_filled": row_filled,
             "needs_guide": wm is not None and wm[1] > 0, "wmedian_takes_codes": wm is not None and keep and not row_filled}
    return {k: bool(v) for k, v in facts.items()}


def test_the_table_has_every_combination():
    keys = set(itertools.product(("off", "on", "fill"), ("off", "on", "fill"), ("off", "fill0", "fill4"), (0, 10)))
    assert set(TABLE) == keys and len(TABLE) == 54
    assert all(len(row) == len(FACTS) and set(row) <= {"T", "."} for row in TABLE.values())


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "-".join(map(str, k)))
def test_derived_facts(key):
    want = {name: c == "T" for name, c in zip(FACTS, TABLE[key])}
    options = Options.make(**flags(*key))
    options.check()
    got = {name: getattr(options, name) for name in FACTS}
    assert all(type(v) is bool for v in got.values()), got
    assert got == want
    assert former_inference(**flags(*key)) == want, "the table is what the inference CLI did"
    ev = former_evaluate(**flags(*key))
    assert ev == {name: want[name] for name in ev}, "the two CLIs agreed on what both express"


def test_options_are_immutable_and_built_from_args_or_keywords():
    p = inference.build_parser()
    args = p.parse_args(["--lr_check", "1", "--lr_fill", "--wmedian", "2"])
    inference.check_lr_arguments(p, args)
    inference.check_wmedian_arguments(p, args)
    options = Options.from_args(args)
    assert options == Options(lr_check=1.0, lr_fill=True, wmedian=2, wmedian_sigma=10.0, wmedian_fill=0)
    assert options == Options.make(lr_check=1, lr_fill=1, speckle=None, speckle_diff=None, wmedian=2, wmedian_sigma=None, wmedian_fill=None)
    assert Options.from_args(p.parse_args([])) == Options() and Options().stages_on == []
    with pytest.raises(AttributeError):
        options.lr_fill = False


def _rejected_values():
    """The argv lists of the speckle and median CPU tests that give a stage a value it does not support (the others are a
    dependent flag without its main flag, and --workers)."""
    speckle = [m.args[1] for m in test_speckle_cpu.test_cli_argument_errors.pytestmark if m.name == "parametrize"][0]
    out = []
    for argv in list(speckle) + test_wmedian_cpu.ARGV_ERRORS:
        main = argv[0] in ("--speckle", "--wmedian") and "--workers" not in argv
        out.append((argv, main))
    return out


def test_check_rejects_what_the_cli_tests_reject():
    cases = _rejected_values()
    values = [argv for argv, is_value in cases if is_value]
    assert len(cases) == 17 and len(values) == 11
    for mod in (inference, evaluate):
        for argv in values:
            args = mod.build_parser().parse_args(argv)
            with pytest.raises(ValueError, match=argv[-2]):
                Options.from_args(args).check()
    for bad in (dict(lr_check=-1.0), dict(lr_check=float("nan")), dict(lr_check=float("inf")), dict(speckle=2 ** 31),
                dict(wmedian=1, wmedian_fill=2 ** 31)):
        with pytest.raises(ValueError):
            Options.make(**bad).check()
    for flag, name in (("lr_check", "--lr_check TAU"), ("occ_check", "--occ_check TAU"), ("speckle_diff", "--speckle_diff D"), ("wmedian_sigma", "--wmedian_sigma S")):
        with pytest.raises(ValueError, match=f"^{name} must be finite and >= 0, got -1.0$"):      # the whole sentence, which the CLIs pass on as it is
            Options.make(**{"speckle": 5, "wmedian": 1, flag: -1}).check()
    Options.make(lr_check=0.0, speckle=2 ** 31 - 1, speckle_diff=0.0, wmedian=3, wmedian_sigma=0.0, wmedian_fill=2 ** 31 - 1).check()
