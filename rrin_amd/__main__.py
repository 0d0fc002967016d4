"""``python -m rrin_amd --model_name M convert --sf S --fps F --image_folder D``

Same command line as the reference (`/root/reference/__main__.py:33-72`).
``train`` is parsed for compatibility but refused: the training loop and its
losses (reference ``train.py`` / ``losses.py``: AdamW, the VGG19 perceptual loss
whose weights come from the network) are out of scope.  The
model's own forward and backward do run on the HIP training kernels
(``rrin_amd.autograd``): call ``Net`` under autograd from your loop.

``python -m rrin_amd --model_name M evaluate --y4m_in clip.y4m|-`` is rrin_amd's own: hold-out PSNR /
SSIM of the model on a clip (``convert.evaluate_y4m``).

``python -m rrin_amd --model_name M finetune --y4m_in clip.y4m|- --steps N`` is rrin_amd's own too:
fine-tuning on the clip's own held-out frames (``finetune.finetune_y4m``); it writes
``models/M<epoch+1:04d>.pth``."""
import argparse
import warnings


def build_parser():
    p = argparse.ArgumentParser(description="RRIN video frame interpolation on MI355X (HIP)")
    p.add_argument("--model_name", type=str, default="Model", required=True, help="Name of model")
    p.add_argument("--no-cuda", action="store_true", default=False, help="disables CUDA")
    p.add_argument("--rm", action="store_true", default=False, help="Removed temp folder on proper finish.")
    sub = p.add_subparsers(dest="mode")
    sub.required = True
    tr = sub.add_parser("train", help="Train the model (the loop is not shipped by rrin_amd: see finetune)")
    tr.add_argument("--train_folder", type=str, required=True)
    tr.add_argument("--resume", action="store_true", default=False)
    tr.add_argument("--batch_size", type=int, default=2)
    cv = sub.add_parser("convert", help="Performs interpolation of a video.")
    cv.add_argument("--input_video", type=str, required=False)
    cv.add_argument("--output_video", type=str, required=False)
    cv.add_argument("--sf", type=int, required=True, help="How many intermediate frames to make.")
    cv.add_argument("--fps", type=str, required=True, help="FPS of output")
    cv.add_argument("--image_folder", type=str, required=False)
    cv.add_argument("--resume", action="store_true", default=False)
    # rrin_amd additions
    cv.add_argument("--batch", type=int, default=4, help="frame pairs per GPU call")
    cv.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"],
                    help="fp32: exact fp32 (default); fp32_split16: fp32-emulated with fp16 hi+lo x3; fp16")
    cv.add_argument("--scene_threshold", type=float, default=None,
                    help="scene gate, off by default: mean absolute byte difference (0-255) above which a pair "
                         "is a shot change and yields the nearer input frame instead of a blend; repeated "
                         "frames are passed through.  No value has been validated on real footage")
    cv.add_argument("--flow_scale", type=int, default=1, choices=[1, 2, 4],
                    help="estimate the flow on frames reduced by this factor and scale it up (large frames, large "
                         "motion); warp, mask and refinement stay at full size.  Quality is not validated: judge "
                         "it with `evaluate --flow_scale`")
    cv.add_argument("--alpha", action="store_true", default=False,
                    help="image folders: read the frames as RGBA and carry the alpha plane along with the picture's "
                         "own motion; the interpolated frames are RGBA PNGs.  RGB is taken as stored (no premultiply); "
                         "one GPU only.  Without it a matte is dropped")
    cv.add_argument("--y4m_in", type=str, default=None, metavar="PATH|-",
                    help="read a Y4M stream (4:2:0, 4:2:2 or 4:4:4 of 8, 10 or 12 bits; \"-\": stdin, e.g. from "
                         "ffmpeg -f yuv4mpegpipe) instead "
                         "of a video or folder; needs --y4m_out.  No PNG folder, no RGB frame: the frames go "
                         "through the network as YUV.  --fps is ignored (the rate comes from the stream)")
    cv.add_argument("--y4m_out", type=str, default=None, metavar="PATH|-",
                    help="write the interpolated Y4M stream here (\"-\": stdout)")
    cv.add_argument("--fps_out", type=str, default=None, metavar="NUM[/DEN]",
                    help="with --y4m_in / --y4m_out: convert the stream's frame rate to this higher rate, e.g. "
                         "60000/1001 or 60 (24 -> 60, 25 -> 30, ...), instead of --sf intermediates per pair; "
                         "needs --sf 0 (with --samples: any rate).  Quality at uneven t has not been validated on "
                         "footage")
    cv.add_argument("--samples", type=int, default=None, metavar="S",
                    help="with --fps_out: a synthetic shutter.  Every output frame is the mean of S (1..256) frames "
                         "interpolated across the shutter window, and --fps_out may be ANY rate, lower ones included "
                         "(60 -> 24, 120 -> 24).  The mean is over code values: no transfer function is applied")
    cv.add_argument("--shutter", type=str, default=None, metavar="NUM/DEN",
                    help="with --samples: the share of an output frame's time the shutter is open, in (0, 1], e.g. "
                         "1/2 (the default, a 180 degree shutter)")
    cv.add_argument("--light", type=str, default=None, choices=["srgb", "bt1886", "gamma22", "pq", "hlg"],
                    help="with --samples (> 1): the transfer curve of the material.  The mean of the samples is then "
                         "taken in linear light, as a shutter integrates it, and encoded back to the nearest code "
                         "value.  Y4M carries no transfer tag, so the curve must be named: no default, no guessing "
                         "(without it the mean stays over code values)")
    cv.add_argument("--shutter_weights", type=str, default=None, choices=["box", "triangle"],
                    help="with --samples (> 1): how the samples of an exposure are weighted.  box: all equal (the "
                         "default); triangle: w_k = min(k + 1, S - k), a shutter that opens and closes gradually")
    ev = sub.add_parser("evaluate", help="Hold-out PSNR / SSIM of the model on a Y4M clip.")
    ev.add_argument("--y4m_in", type=str, required=True, metavar="PATH|-",
                    help="the clip: a Y4M stream of any format convert --y4m_in takes (\"-\": stdin)")
    ev.add_argument("--hold", type=int, default=2,
                    help="every hold-th frame is an input; the hold-1 frames between two inputs are dropped, "
                         "interpolated back and compared with the originals (default 2)")
    ev.add_argument("--batch", type=int, default=4, help="held-out frames per GPU call")
    ev.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"])
    ev.add_argument("--scene_threshold", type=float, default=None,
                    help="scene gate as in convert (off by default); the report counts cut and duplicate pairs")
    ev.add_argument("--flow_scale", type=int, default=1, choices=[1, 2, 4],
                    help="as in convert: the Flow U-Net at 1/s of the frame size; the report records it")
    ev.add_argument("--report", type=str, default=None, metavar="PATH",
                    help="write every row and the summary here as JSON (the summary is printed either way)")
    ft = sub.add_parser("finetune", help="Fine-tune the model on a Y4M clip's own held-out frames.")
    ft.add_argument("--y4m_in", type=str, required=True, metavar="PATH|-",
                    help="the clip: a Y4M stream of any format convert --y4m_in takes (\"-\": stdin); it is kept "
                         "on the device as a whole")
    ft.add_argument("--steps", type=int, required=True, help="optimiser steps")
    ft.add_argument("--batch", type=int, default=2, help="triplets per step (default 2, the reference's batch)")
    ft.add_argument("--crop", type=int, default=256, help="side of the square training crop, a multiple of 16")
    ft.add_argument("--spans", type=_spans, default=(2,), metavar="2,3,4",
                    help="frame distances between the two inputs of a triplet; the first is also the hold of the "
                         "validation (default 2)")
    ft.add_argument("--lr", type=float, default=1e-4, help="AdamW learning rate (default 1e-4, the reference's)")
    ft.add_argument("--seed", type=int, default=0, help="seed of the triplet schedule")
    ft.add_argument("--scene_threshold", type=float, default=None,
                    help="scene gate as in convert (off by default): cut and duplicate pairs give no triplet")
    ft.add_argument("--val_fraction", type=float, default=0.1,
                    help="share of the clip's last frames that is never trained on and measured before and after")
    ft.add_argument("--no_augment", action="store_true", default=False,
                    help="no random crop origin, flip or time reversal")
    ft.add_argument("--report", type=str, default=None, metavar="PATH",
                    help="write the losses, the schedule and both validations here as JSON")
    ft.add_argument("--vgg_weights", type=str, default=None, metavar="PATH",
                    help="a VGG19 state dict on disk (torchvision's vgg19-*.pth; keys features.N.weight/bias or "
                         "N.weight/bias): adds the reference's perceptual term, w_vgg * ||VGG19[:relu4_4](out) - "
                         "VGG19[:relu4_4](truth)||, to the loss.  The file is never downloaded; a missing or "
                         "mismatching one is an error before the clip is read")
    ft.add_argument("--w_vgg", type=float, default=0.1,
                    help="weight of the perceptual term (default 0.1, the reference's CombinedLoss / 10)")
    ft.add_argument("--vgg_cfg", type=_vgg_cfg, default=None, metavar="64,64,M,...",
                    help="the conv stack the weights file is checked against, output channels and M for a 2x2 "
                         "max pool (default: VGG19 up to relu4_4; other stacks are for tests)")
    return p


def _vgg_cfg(text):
    """``4,4,M,8`` -> (4, 4, "M", 8)."""
    try:
        cfg = tuple("M" if v.strip() == "M" else int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"a conv stack is comma-separated ints and M, got {text!r}")
    if not cfg or cfg.count("M") != 3 or any(v != "M" and v < 1 for v in cfg):
        raise argparse.ArgumentTypeError(f"a conv stack has positive widths and three M, got {text!r}")
    return cfg


def _spans(text):
    """``2,3,4`` -> (2, 3, 4)."""
    try:
        spans = tuple(int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"spans are comma-separated ints, got {text!r}")
    if not spans or any(s < 2 for s in spans):
        raise argparse.ArgumentTypeError(f"spans are ints >= 2, got {text!r}")
    return spans


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == "evaluate":
        from .convert import evaluate
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=UserWarning)
            evaluate(args)
        return
    if args.mode == "finetune":
        from .finetune import finetune
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=UserWarning)
            finetune(args)
        return
    if args.mode == "train":
        raise SystemExit("rrin_amd does not ship the training loop (AdamW, VGG19 perceptual loss: out of "
                         "scope, SURVEY §2 rows 11-12); Net.forward / backward run on the HIP training "
                         "kernels under autograd, so drive them from your own loop or the reference train.py")
    from .convert import convert
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=UserWarning)
        convert(args)


if __name__ == "__main__":
    main()
