#!/usr/bin/env python
"""Golden vectors for BVH ingestion (qpgesture_amd/process_bvh.py) by running the REFERENCE's own `pymo` classes and scipy
on small synthetic BVH files: the parser (pymo/parsers.py), the pipeline of process/beat_data_to_lmdb.py:58-65
(DownSampler, RootTransformer('hip_centric'), Mirror('X'), JointSelector, ConstantsRemover, Numpyfier) and the
Rotation.from_euler('ZXY') loop of :79-86, assembled here from `pymo` directly because that module itself also imports
librosa and lmdb.  `pymo.preprocessing` imports transforms3d, which this path never calls: an empty stand-in module is
registered before the import.

The BVH text is this repository's (tests/bvh_ref.py:bvh_text): Hips with 6 channels, the 15 target joints, one finger per
hand, legs, end sites; 41 frames at 120 fps (T = 20 at 60 fps, T = 7 at 20 fps); angles uniform in +-170 degrees with
some planted at exactly 0, +-90 and +-180.  One file names its channels Zrotation Xrotation Yrotation, the other
Xrotation Yrotation Zrotation: the reference applies 'ZXY' to whatever order the file has and mirrors by channel NAME.
Each fixture stores the file's bytes, the parser's values and upper / upper_mirror at both rates.

Usage: python tests/golden/make_golden_bvh_features.py <path of the reference checkout>
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

FIXTURES = {"bvh_features_zxy": ("ZXY", 61), "bvh_features_xyz": ("XYZ", 62)}     # name: (channel order, seed)
FRAMES = 41


def reference_features(path, fps, joints):
    from pymo.parsers import BVHParser
    from pymo.preprocessing import ConstantsRemover, DownSampler, JointSelector, Mirror, Numpyfier, RootTransformer
    from scipy.spatial.transform import Rotation as R
    from sklearn.pipeline import Pipeline
    parsed = BVHParser().parse(path)
    data_pipe = Pipeline([                                                # beat_data_to_lmdb.py:58-65
        ('dwnsampl', DownSampler(tgt_fps=fps, keep_all=False)),
        ('root', RootTransformer('hip_centric')),
        ('mir', Mirror(axis='X', append=True)),
        ('jtsel', JointSelector(joints, include_root=True)),
        ('cnst', ConstantsRemover()),
        ('np', Numpyfier())
    ])
    out_data = data_pipe.fit_transform([parsed])
    assert out_data[0].shape[1] == len(joints) * 3, out_data.shape
    out_data = out_data.reshape((out_data.shape[0], out_data.shape[1], -1, 3))                       # :80-86
    out_matrix = np.zeros((out_data.shape[0], out_data.shape[1], out_data.shape[2], 9))
    for i in range(out_data.shape[0]):
        for j in range(out_data.shape[1]):
            r = R.from_euler('ZXY', out_data[i, j], degrees=True)
            out_matrix[i, j] = r.as_matrix().reshape(out_data.shape[2], 9)
    out_matrix = out_matrix.reshape((out_data.shape[0], out_data.shape[1], -1))
    return parsed.values.values, out_matrix[0], out_matrix[1]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.modules.setdefault("transforms3d", types.ModuleType("transforms3d"))
    sys.path.insert(0, os.path.join(sys.argv[1], "process"))
    from tests import bvh_ref
    for name, (order, seed) in FIXTURES.items():
        rng = np.random.Generator(np.random.PCG64(seed))
        values = bvh_ref.planted_angles(rng, FRAMES, bvh_ref.n_channels())
        data = bvh_ref.bvh_text(values, order=order).encode()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, name + ".bvh")
            with open(path, "wb") as f:
                f.write(data)
            vals, up60, um60 = reference_features(path, 60, bvh_ref.TARGET_JOINTS)
            _, up20, um20 = reference_features(path, 20, bvh_ref.TARGET_JOINTS)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), bvh=np.frombuffer(data, np.uint8), values=vals,
                            upper_60=up60, upper_mirror_60=um60, upper_20=up20, upper_mirror_20=um20)
        print(name, "bytes", len(data), "values", vals.shape, "upper", up60.shape, up20.shape)


if __name__ == "__main__":
    main()
