"""python -m gauspcc_amd.cli.train: train GausPcgc's context network on gfx950 (the flags of src/ai_pcc/GausPcgc/train.py:42-59).

Clouds are read with cli/io.py's readers, quantised as the codec CLIs do (`xyz / 0.001 + 131072` unless --is_data_pre_quantized,
then rounded) and deduplicated.  A cloud above --max_num points is cut into parts by recursive median halving on its axis of largest
variance, and every step takes one random part (the reference's patch dataset).  Adam; `ckpt_*.pt`, `best_model_*.pt` and
`final_model_*.pt` are plain state dicts with the upstream keys, which the compress / decompress CLIs load as they are."""
import argparse
import glob
import os
import random
import time

import numpy as np
import torch

from .io import read_points


def split_patches(points: np.ndarray, max_num: int):
    """Parts of at most max_num points: halve at the median of the axis of largest variance until every part fits.  Deterministic;
    the parts partition the input."""
    out, todo = [], [np.asarray(points)]
    while todo:
        p = todo.pop()
        if p.shape[0] <= max_num:
            out.append(p)
            continue
        ax = int(np.argmax(p.astype(np.float64).var(axis=0)))
        order = np.argsort(p[:, ax], kind="stable")
        h = p.shape[0] // 2
        todo += [p[order[h:]], p[order[:h]]]
    return out


def load_cloud(path: str, pre_quantized: bool) -> np.ndarray:
    xyz = np.asarray(read_points(path), dtype=np.float64)
    if not pre_quantized:
        xyz = xyz / 0.001 + 131072
    return np.unique(np.round(xyz).astype(np.int32), axis=0)


def _str2bool(v):
    return str(v).lower() in ("1", "true", "yes", "y")


def parser():
    p = argparse.ArgumentParser(prog="gauspcc_amd.cli.train", description="Training from scratch.", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--training_data", default="./Dataset/KITTI_detection/training/velodyne/*.ply", help="Training data (Glob pattern).")
    p.add_argument("--val_data", default="", help="Validation data (Glob pattern).")
    p.add_argument("--model_save_folder", default="./model/KITTIDetection", help="Directory where to save trained models.")
    p.add_argument("--is_data_pre_quantized", type=_str2bool, default=False, help="Whether the training data is pre quantized.")
    p.add_argument("--channels", type=int, default=32, help="Neural network channels (32: the MFMA path).")
    p.add_argument("--kernel_size", type=int, default=3, help="Convolution kernel size.")
    p.add_argument("--batch_size", type=int, default=1, help="Clouds per step (one after the other).")
    p.add_argument("--learning_rate", type=float, default=0.0005, help="Learning rate.")
    p.add_argument("--lr_decay", type=float, default=0.1, help="Decays the learning rate to x times the original.")
    p.add_argument("--lr_decay_steps", type=lambda s: [int(v) for v in str(s).strip("[]").split(",") if v.strip()], default=[40000, 90000],
                   help="Decays the learning rate at these steps (comma separated).")
    p.add_argument("--max_steps", type=int, default=110000, help="Train up to this number of steps.")
    p.add_argument("--val_interval", type=int, default=500, help="Validate every N steps.")
    p.add_argument("--log_interval", type=int, default=100, help="Log training info every N steps.")
    p.add_argument("--max_num", type=int, default=150000, help="Largest training part (points).")
    p.add_argument("--stage", default="ue_4stage_conv", help="Name used in the checkpoint file names.")
    p.add_argument("--seed", type=int, default=11)
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    from ..pcgc_net import Network

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    files = sorted(glob.glob(args.training_data, recursive=True))
    if not files:
        raise SystemExit(f"no training data matches {args.training_data!r}")
    val_files = sorted(glob.glob(args.val_data, recursive=True)) if args.val_data else []
    os.makedirs(args.model_save_folder, exist_ok=True)
    parts = [split_patches(load_cloud(f, args.is_data_pre_quantized), args.max_num) for f in files]
    val = [load_cloud(f, args.is_data_pre_quantized) for f in val_files]
    dev = torch.device("cuda")
    net = Network(args.channels, args.kernel_size).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=args.learning_rate)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=args.lr_decay_steps, gamma=args.lr_decay)
    print(f"training set {len(files)} clouds, validation set {len(val)}; parameters {sum(p.numel() for p in net.parameters()):,}", flush=True)
    best, losses, t0 = float("inf"), [], time.time()
    for step in range(1, args.max_steps + 1):
        bits, n = 0.0, 0
        opt.zero_grad()
        for _ in range(args.batch_size):
            pp = parts[random.randrange(len(parts))]
            c = torch.from_numpy(pp[random.randrange(len(pp))]).to(dev)
            b = net.cloud_bits(c)
            bits, n = bits + b, n + c.shape[0]
        loss = bits / n
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.item())
        if step % args.log_interval == 0:
            print(f"step {step} loss {np.mean(losses):.5f} lr {opt.param_groups[0]['lr']:.6f} ({time.time() - t0:.1f} s)", flush=True)
            losses = []
        if step % args.val_interval == 0 or step == args.max_steps:
            torch.save(net.state_dict(), os.path.join(args.model_save_folder, f"ckpt_{args.stage}.pt"))
            if val:
                with torch.no_grad():
                    v = float(np.mean([net(torch.from_numpy(c).to(dev)).item() for c in val]))
                print(f"step {step} validation bpp {v:.5f}", flush=True)
                if v < best:
                    best = v
                    torch.save(net.state_dict(), os.path.join(args.model_save_folder, f"best_model_{args.stage}.pt"))
    torch.save(net.state_dict(), os.path.join(args.model_save_folder, f"final_model_{args.stage}.pt"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
