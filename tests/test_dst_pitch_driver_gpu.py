"""The Fortran driver's device flow with pitched results: float32 big-endian fields whose only reader is the file writer (and U / V of
the wind chain) are regridded into level planes on whole 128-byte lines and written with mpg_dev_to_file_planes.  On the 151 x 91
namelist (150 x 90 mass points: every dense float32 plane starts 112 bytes further into a line) the output file must be the one the
dense layout writes (MPASSIT_DST_PITCH=0), byte for byte -- with one image, and with two images writing their row blocks level by level."""
import os
import subprocess

import pytest

from test_fortran_driver import NAMELIST, _driver
from test_fortran_driver_nc_gpu import _write_inputs

PITCHED = "FLOAT32 RESULTS ON PITCHED LEVEL PLANES"

pytestmark = pytest.mark.gpu


def test_pitched_device_flow_writes_the_dense_file(tmp_path, gpu_lib, regional_case, monkeypatch):
    m, g = regional_case
    assert ((g.nx * g.ny) * 4) % 128 != 0
    d = str(tmp_path)
    _write_inputs(d, m, 6, 4)
    nml = NAMELIST.format(d=d).replace(".raw", ".nc")
    outs = {}
    for name, pitch in (("dense", "0"), ("pitched", "1")):
        open(os.path.join(d, "namelist.%s" % name), "w").write(nml.replace("out.nc", "out_%s.nc" % name))
        r = subprocess.run([_driver(), "namelist.%s" % name], cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, MPASSIT_DST_PITCH=pitch))
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FIELDS STAY ON THE DEVICE" in r.stdout
        assert (PITCHED in r.stdout) == (pitch == "1"), "the driver did not take the %s path" % name
        outs[name] = open(os.path.join(d, "out_%s.nc" % name), "rb").read()
    assert len(outs["dense"]) == len(outs["pitched"]) and outs["dense"] == outs["pitched"]
    # two images, pitched: each writes its rows of every level from its own planes
    open(os.path.join(d, "namelist.two"), "w").write(nml.replace("out.nc", "out_two.nc"))
    monkeypatch.setenv("MPASSIT_DST_PITCH", "1")
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mpassit_ranks
    res = mpassit_ranks.launch("namelist.two", 2, gpus=1, exe=_driver(), cwd=d, timeout=600)
    for rank, (code, so, se) in enumerate(res):
        assert code == 0, "image %d: %s\n%s" % (rank, so[-2000:], se[-2000:])
        assert PITCHED in so, "image %d did not pitch" % rank
    assert open(os.path.join(d, "out_two.nc"), "rb").read() == outs["dense"]
