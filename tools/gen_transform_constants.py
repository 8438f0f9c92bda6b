"""Writes gaussian-splatting-slam_amd/csrc/transform_constants.inc: the SH sample directions and the inverses of their basis
matrices that csrc/transform.hip bakes in (scene_utils/sh_rotation.py holds the directions).  Run after changing them:
    python tools/gen_transform_constants.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

from scene_utils.sh_rotation import constants_text  # noqa: E402

if __name__ == "__main__":
    path = os.path.join(ROOT, "gaussian-splatting-slam_amd", "csrc", "transform_constants.inc")
    with open(path, "w") as f:
        f.write(constants_text())
    print("wrote", path)
