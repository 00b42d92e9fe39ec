"""--auto-exposure [P] of the command line (fractal-renderer_amd/cli/fractal_cli.cpp): the file it writes is Python's
get_image_auto of the same view, the exposure it prints is auto_exposure's; it is refused beside -e, more than one device and
the fern, each with its own message (those need no device)."""
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_cpp_host import CLI_EXE, _read_ppm, build_cli


@pytest.fixture(scope="module")
def cli():
    build_cli()
    return CLI_EXE


def test_the_three_refusals(cli):
    for args, msg in [(["--auto-exposure", "-e", "3"], "does not combine with -e / --exposure"),
                      (["--exposure", "3", "--auto-exposure", "0.5"], "does not combine with -e / --exposure"),
                      (["--auto-exposure", "--devices", "0,1"], "runs on one device"),
                      (["--auto-exposure", "-a", "fern"], "does not apply to -a fern"),
                      (["--auto-exposure=2"], "percentile within [0, 1]")]:
        r = subprocess.run([cli] + args + ["64", "48"], capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)


# the Misiurewicz point i at 1e18: the neighbourhood of tests/deep_edge_views.py's deep views, which escapes in a narrow band
DEEP = ["--perturbation", "-x", "0", "-y", "1.0000000000000000000000000000000", "-s", "1e18", "-i", "3000"]


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["plain", "perturbation"])
@pytest.mark.parametrize("flag", [["--auto-exposure"], ["--auto-exposure", "1.0"]], ids=["default", "p1"])
def test_the_cli_writes_get_image_auto(cli, tmp_path, view, flag):
    import fractal_renderer_amd as fr

    p = float(flag[1]) if len(flag) > 1 else 0.99
    if view == "plain":
        args, kw = ["-i", "300"], dict()
        cfg = fr.Config.from_buffer_copy(bytes(O.cli_config(64, 48, iterations=300)))
    else:
        args = DEEP
        cfg = fr.Config.from_buffer_copy(bytes(O.cli_config(64, 48, iterations=3000, scale=(1e18, 1e18))))
        kw = dict(precision=fr.Precision.PT, centre=fr.WideCentre.from_str(DEEP[2], DEEP[4], scale=1e18))
    out = str(tmp_path / "auto")
    r = subprocess.run([cli] + args + flag + ["64", "48", "-o", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    image, exposure = fr.get_image_auto(cfg, percentile=p, **kw)
    assert np.array_equal(_read_ppm(out + ".ppm"), image)
    printed = re.search(r"auto-exposure (\S+) \(percentile (\S+) of the escape indices\)", r.stdout)
    assert printed and float(printed.group(1)) == exposure and float(printed.group(2)) == p
    z, it = fr.escape_rows(cfg, **kw)
    assert exposure == fr.auto_exposure(cfg, fr.view_stats(cfg, z, it), p) and exposure != cfg.exposure
    quiet = subprocess.run([cli] + args + flag + ["64", "48", "-o", out, "--quiet"], capture_output=True, text=True, timeout=120)
    assert quiet.returncode == 0 and quiet.stdout == ""
