"""Writes tests/golden/three_view_default.npz: one triple of 1 150 common matches (the first of tools/bench_three_view.py's) and
what the host build of include/akz_three_view_math.h (tests/cpp/three_view_host.c) makes of it at the reference's default
settings — 9 runs of 65 536 iterations on 1 024 landmarks, about three minutes on one core.  tests/test_gpu_three_view.py
holds the device to it bit for bit.

    python tests/golden/make_three_view_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import three_view_checker as K  # noqa: E402

CAP = 1280


def main():
    rig = K.Rig(9000, 1150, noise=0.5, perturb=2e-3, n_first=60, n_second=60, outliers=40)
    kps, triples, fo, so = rig.scene_arrays(CAP, shuffle_seed=0)
    h = K.init_scene(kps, 3, [0, 1, 2], K.rig_camera(), rig.pose_in, triples, rig.n, fo, rig.n_first, so, rig.n_second, K.settings())
    np.savez_compressed(os.path.join(HERE, "three_view_default.npz"), kps=kps.view(np.uint8).reshape(3, CAP, 28), triples=triples, first_only=fo,
                        second_only=so, counts=np.array([rig.n, rig.n_first, rig.n_second], np.uint32), pose_in=rig.pose_in,
                        verdict=np.uint32(h["verdict"]), stats=h["stats"], pose_out=h["pose_out"], combined=h["combined"],
                        first_ok=h["first_ok"], second_ok=h["second_ok"])
    print("verdict", h["verdict"], "stats", h["stats"].tolist())


if __name__ == "__main__":
    main()
