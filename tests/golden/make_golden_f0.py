#!/usr/bin/env python
"""Generate tests/golden/continuous_f0.npz by IMPORTING THE REFERENCE's ``crank.utils.convert_continuos_f0``.

Runs only in the authoring container (needs /root/reference).  Nothing from the reference is copied: the fixture holds
F0 contours made here and what the imported function returned for them, plus ``lf0`` / ``lcf0`` formed as
crank/feature/feature.py:86-88 forms them (numpy.log of the function's in-place modified input plus 1e-10, and of its
continuous contour).  Packages the reference's module imports but this container lacks are import-only placeholders, as
in make_golden.py; the function under test uses numpy and scipy.interpolate only.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_f0.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


for name in ("librosa", "soundfile", "sprocket", "h5py"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            _placeholder(name)
if not hasattr(sys.modules["sprocket"], "__file__"):
    sys.modules["sprocket"].speech = _placeholder("sprocket.speech", Synthesizer=None, FeatureExtractor=None)
    sys.modules["sprocket"].util = _placeholder("sprocket.util", HDF5=None)

from crank.utils import convert_continuos_f0  # noqa: E402

EPS = 1e-10  # crank/feature/feature.py


def contours():
    rng = np.random.default_rng(7)
    out = []
    f = 120.0 + 30.0 * np.sin(np.arange(200) / 9.0) + rng.uniform(-2, 2, 200)
    for a, b in ((0, 7), (40, 55), (56, 57), (120, 160), (190, 200)):
        f[a:b] = 0.0
    out.append(f)  # unvoiced at both ends, gaps of 1 .. 40 frames
    out.append(rng.uniform(80, 300, 64))  # voiced throughout
    f = np.zeros(50)
    f[23] = 211.25
    out.append(f)  # one voiced frame
    f = rng.uniform(80, 300, 90)
    f[rng.uniform(size=90) < 0.5] = 0.0
    f[0], f[-1] = 150.5, 99.75
    out.append(f)  # voiced first and last frame
    # the first voiced value returns later and the last voiced value occurs earlier: the reference looks both up by value
    f = np.zeros(80)
    f[10:30] = 140.0
    f[30:50] = np.linspace(141.0, 160.0, 20)
    f[60:70] = 140.0
    out.append(f)
    f = np.zeros(70)
    f[5:20] = 100.0 + np.arange(15.0)
    f[30:40] = 180.0
    f[50:60] = 180.0
    out.append(f)
    out.append(np.array([0.0, 0.0, 133.0, 0.0, 171.0, 0.0]))
    return out


def main():
    data = {}
    for k, f in enumerate(contours()):
        data[f"in_{k}"] = f.copy()
        g = f.copy()
        uv, cf0 = convert_continuos_f0(g)  # overwrites the ends of g
        data[f"uv_{k}"] = uv
        data[f"f0_{k}"] = g
        data[f"cf0_{k}"] = np.asarray(cf0, np.float64)
        data[f"lf0_{k}"] = np.log(g + EPS)
        data[f"lcf0_{k}"] = np.log(cf0)
    path = os.path.join(HERE, "continuous_f0.npz")
    np.savez(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
