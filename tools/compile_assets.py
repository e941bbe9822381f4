"""Compile the reference's Adroit MJCF into the committed model tables (models/*.npz) and
their appearance parts (tests/golden/appearance_*.npz) and camera tables
(tests/golden/cameras_*.npz).

Run in the build container (where /root/reference exists):
    python tools/compile_assets.py [--assets DIR]
The GPU box has no /root/reference; it loads the committed .npz tables.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mj_envs_amd.mjcf import compile_mjcf  # noqa: E402
from mj_envs_amd.tasks import APPEARANCE_DIR, MODEL_DIR, TASKS, appearance_path, cameras_path  # noqa: E402

DEFAULT_ASSETS = "/root/reference/mj_envs_vision/hand_manipulation_suite/assets"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", default=os.environ.get("ADROIT_ASSETS", DEFAULT_ASSETS))
    args = ap.parse_args()
    os.makedirs(MODEL_DIR, exist_ok=True)
    for spec in TASKS.values():
        m = compile_mjcf(os.path.join(args.assets, spec.xml))
        out = os.path.join(MODEL_DIR, spec.xml.replace(".xml", ".npz"))
        m.save_npz(out)
        os.makedirs(APPEARANCE_DIR, exist_ok=True)
        m.save_npz(appearance_path(spec.xml), appearance=True)     # colours, materials, lights
        m.save_cameras(cameras_path(spec.xml))                     # names, bodies, poses, fovy
        print(spec.env_id, m.dims, "->", out, appearance_path(spec.xml), cameras_path(spec.xml))


if __name__ == "__main__":
    main()
