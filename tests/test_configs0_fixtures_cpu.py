"""CPU: the configs[0] data fixtures (tests/golden/configs0/) are the reference's own files -- checked byte for byte against the
SHA-256 digests of the reference's files, recorded when the fixtures were taken -- and their content is what the tests expect."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "configs0")
# SHA-256 of the reference's config/kitti_stereo.cfg, and of the first 12 lines of its data/kitti_init_poor/00.txt (4541 lines)
REF_SHA256 = {
    "config/kitti_stereo.cfg": "f9290f725720cbd3950a61f143c96610918e28efb343fa50aef0d3ed76d0436e",
    "data/kitti_init_poor/00.txt": "6009326431529753b9d93d64d0ba8b8bd2c7bb91dbf5a58f21744b6c1b8c71d6",
}


def test_fixture_content():
    import re
    text = open(os.path.join(FIX, "config", "kitti_stereo.cfg")).read()
    keys = dict(re.findall(r"^(\w+)\s*=\s*(\S+)\s*$", text, flags=re.M))
    assert keys["slidingWindowSize"] == "5" and keys["patchRadius"] == "1" and keys["maxNumPoints"] == "4096"
    assert keys["minScore"] == "0.65" and keys["robustThreshold"] == "0.05"
    assert keys["Trajectory"] == "../data/kitti_init_poor/00.txt"
    poses = np.loadtxt(os.path.join(FIX, "data", "kitti_init_poor", "00.txt")).reshape(-1, 3, 4)
    assert poses.shape[0] == 12
    assert np.array_equal(poses[0], np.eye(4)[:3])
    # frame-to-frame poses of a forward-driving car: ~0.7 m per frame along -z (inverse of the motion), tiny rotations
    assert np.all(poses[1:, 2, 3] < -0.6) and np.all(poses[1:, 2, 3] > -0.9)
    assert np.abs(poses[:, :, :3] - np.eye(3)).max() < 0.02


def test_fixtures_are_the_reference_files():
    for rel, digest in REF_SHA256.items():
        with open(os.path.join(FIX, *rel.split("/")), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == digest, rel
