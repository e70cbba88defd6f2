"""The release library has no diagnostic switch (csrc/tuning.h): a process that inherits every one of them from somebody's
tuning shell writes the same files as any other.  One fresh child interpreter (tests/tuning_switches_child.py) runs with the
five switches set that change what a tuning build computes or launches; its .cct files must be the oracle's, its JPEG 2000
files the model's, and both round trips exact.  (Before the gate, CCT_J2K_STAGES=1 cut the JPEG 2000 files short with
status OK.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg2000_model as m
import tuning_switches_child as child

pytestmark = pytest.mark.gpu

SWITCHES = {"CCT_STREAM_DBG": "2", "CCT_STREAM_STAMPS": "1", "CCT_INF_PROF": "1", "CCT_J2K_STAGES": "1", "CCT_J2K_DEC_STAGES": "1"}


def test_release_library_ignores_every_switch(tmp_path):
    from oracle import oracle
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, **SWITCHES)
    env.pop("CCT_HIP_LIB", None)   # the release library, whatever build the suite itself runs
    r = subprocess.run([sys.executable, child.__file__, out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "stream stamps" not in r.stderr and "inflate prof" not in r.stderr   # nothing diagnostic was launched
    slices, frames = child.inputs()
    got = np.load(out)
    for i in range(2):
        assert got[f"cct{i}"].tobytes() == oracle.encode(slices[i]), i
        assert got[f"j2k{i}"].tobytes() == m.encode(frames[i], 16, 0, 2, 32), i
    assert np.array_equal(got["back"], slices)
    assert np.array_equal(got["jback"], frames)
