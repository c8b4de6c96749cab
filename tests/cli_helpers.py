"""What the CPU tests of the inference CLI's flags share: a camera on the command line, the stderr of a command line that main()
refuses before any model or GPU work, and the folder (empty image files) and poses file of a sequence that only the flag checks see."""
import os

import pytest

import temporal_reference as T

CAMERA = ["--camera", "700", "700", "600", "180", "0.5"]


def cli_refused(argv, capsys):
    from lwsnet_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(argv + ["--synthetic_weights"])
    assert e.value.code != 0
    return capsys.readouterr().err


def poses_file(path, n):
    path.write_text("".join(" ".join(str(float(v)) for v in T.forward_pose(k, 0.5).reshape(12)) + "\n" for k in range(n)))
    return str(path)


def sequence_dir(tmp_path, pairs):
    for side in ("image_2", "image_3"):
        os.makedirs(tmp_path / "seq" / side)
        for k in range(pairs):
            (tmp_path / "seq" / side / f"{k:06d}.png").write_bytes(b"")
    return ["--img_path", str(tmp_path / "seq"), "--save_path", str(tmp_path / "out")]
