"""Export a trained generator for inference (the deployment step of the reference's bin/save_model.py).

    python bin/save_model.py <model name> <ckpt dir> <mean_x> <std_x> <mean_y> <std_y> <image size> <is3d 1|0>

Writes <model name>/generator_g.pt and <model name>/meta.json through transfer_em_amd.utils.save_model; the directory
is what predict_cube_from_saved_model and predict_volume_from_saved_model read.  Example:

    python bin/save_model.py trained_example ./checkpoints/train_hemi2hemi/ckpt-1 0.198 0.182 0.067 0.378 132 1
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv):
    if len(argv) != 8:
        sys.exit(__doc__)
    name, ckpt_dir = argv[0], argv[1]
    meanstd_x = (float(argv[2]), float(argv[3]))
    meanstd_y = (float(argv[4]), float(argv[5]))
    size = int(argv[6])
    if argv[7] not in ("0", "1"):
        sys.exit(f"is3d must be 1 or 0, got {argv[7]!r}")
    from transfer_em_amd.utils import save_model
    save_model(name, ckpt_dir, meanstd_x, meanstd_y, size, argv[7] == "1")


if __name__ == "__main__":
    main(sys.argv[1:])
