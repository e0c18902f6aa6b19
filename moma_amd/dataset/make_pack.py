"""Build a data pack from a folder of images (see dataset/pack.py for the format):

    python -m moma_amd.dataset.make_pack --src ROOT --out PACK --resize 512 [--center_crop S] [--chunk 256]

ROOT/{train,val[,test]}/<class name>/* in any format PIL opens.  Classes are numbered by sorted name."""
import argparse

from .pack import build_pack


def main(argv=None):
    p = argparse.ArgumentParser("make_pack")
    p.add_argument("--src", required=True, help="ROOT of the image tree")
    p.add_argument("--out", required=True, help="directory of the pack")
    p.add_argument("--resize", type=int, default=512, help="Resize(size) of the reference's transforms: the smaller edge")
    p.add_argument("--center_crop", type=int, default=None, help="side of the common centre crop (default: --resize)")
    p.add_argument("--chunk", type=int, default=256, help="images decoded per write")
    a = p.parse_args(argv)
    meta = build_pack(a.src, a.out, a.resize, a.center_crop, a.chunk)
    print("packed", {k: v for k, v in meta.items() if k in ("n_cls", "classes", "H", "W", "splits")})


if __name__ == "__main__":
    main()
