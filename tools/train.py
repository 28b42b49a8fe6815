"""Train or evaluate on image files, with the argument names of the reference's train.py (there is no --config-file: every key is a
`KEY VAL` override, mvlpt_amd.config).  The datasets come from DATASET.SOURCES (mvlpt_amd.data), e.g. one CoOp dataset, 16 shots:

    python tools/train.py --trainer MVLPT --output-dir out/pets --seed 1 --clip-weights ViT-B-16.pt \\
        DATASET.SOURCES '[["OxfordPets", "data/oxford_pets/split_zhou_OxfordPets.json", "data/oxford_pets/images"]]' \\
        DATASET.NUM_SHOTS 16 TRAINER.MVLPT.COOP.N_CTX 16 OPTIM.MAX_EPOCH 50 DATALOADER.TRAIN_X.BATCH_SIZE 32

and afterwards `--eval-only --model-dir out/pets --load-epoch 50` on the same sources.  Without --clip-weights the frozen CLIP is the
synthetic one of the named architecture (the weights are not downloaded here)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRAINERS = ("MVLPT", "CoCoOp", "ZeroshotCLIP", "ZeroshotCLIP2", "TPT", "TipAdapter")
EVAL_ONLY_TRAINERS = ("ZeroshotCLIP", "ZeroshotCLIP2", "TPT")         # nothing is trained: test() straight away


def trainer_class(name: str):
    """The trainer class of `--trainer name`."""
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.tip_adapter import TipAdapter
    from mvlpt_amd.tpt import TPT
    from mvlpt_amd.trainer import MVLPT
    from mvlpt_amd.zsclip import ZeroshotCLIP, ZeroshotCLIP2
    return {"MVLPT": MVLPT, "CoCoOp": CoCoOp, "ZeroshotCLIP": ZeroshotCLIP, "ZeroshotCLIP2": ZeroshotCLIP2, "TPT": TPT,
            "TipAdapter": TipAdapter}[name]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trainer", default="MVLPT", choices=list(TRAINERS), help="name of trainer")
    ap.add_argument("--output-dir", default="", help="output directory")
    ap.add_argument("--seed", type=int, default=-1, help="only positive value enables a fixed seed")
    ap.add_argument("--eval-only", action="store_true", help="evaluation only")
    ap.add_argument("--model-dir", default="", help="load model from this directory for eval-only mode")
    ap.add_argument("--load-epoch", type=int, default=None, help="load model weights at this epoch for evaluation")
    ap.add_argument("--backbone", default="", help="MODEL.BACKBONE.NAME")
    ap.add_argument("--clip-weights", default="", help="a CLIP state dict (torch.save of model.state_dict(), or a TorchScript archive)")
    ap.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="modify config options using the command-line")
    args = ap.parse_args()

    import torch

    from mvlpt_amd.config import get_cfg_default

    cfg = get_cfg_default()
    cfg.TRAINER.NAME = args.trainer
    if args.output_dir:
        cfg.OUTPUT_DIR = args.output_dir
    if args.seed >= 0:
        cfg.SEED = args.seed
    if args.backbone:
        cfg.MODEL.BACKBONE.NAME = args.backbone
    cfg.merge_from_list(args.opts or [])
    if not cfg.DATASET.SOURCES:
        raise SystemExit("DATASET.SOURCES is empty: give '[[\"task\", \"split.json or empty\", \"image folder\"], ...]'")
    cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK or len(cfg.DATASET.SOURCES) > 1
    torch.manual_seed(cfg.SEED)               # the prompt initialisation draws from the global generator (train.py: set_random_seed)
    sd = None
    if args.clip_weights:
        try:
            sd = torch.jit.load(args.clip_weights, map_location="cpu").state_dict()
        except RuntimeError:
            sd = torch.load(args.clip_weights, map_location="cpu")
            sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
    trainer = trainer_class(args.trainer)(cfg, clip_state_dict=sd)
    sets = getattr(trainer.dm, "image_sets", {})
    print("resident on the device: " + ", ".join(f"{k} {s.resident_bytes / 2 ** 20:.1f} MiB ({s.n_device} device, {s.n_host} host, "
                                                   f"{s.n_corrupt} corrupt)" if s is not None else f"{k} streams" for k, s in sets.items()))
    if args.eval_only or args.trainer in EVAL_ONLY_TRAINERS:
        trainer.load_model(args.model_dir, epoch=args.load_epoch)
        print(f"{cfg.TEST.SPLIT}: {trainer.test():.4f}  {trainer.last_task_results or ''}")
        return
    result = trainer.train()
    if not cfg.TEST.NO_TEST:
        print(f"{cfg.TEST.SPLIT}: {trainer.last_results}  {trainer.last_task_results or ''}")
    return result


if __name__ == "__main__":
    main()
