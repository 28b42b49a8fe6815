"""What the loaders of mvlpt_amd.data cost on one GPU.
Input: synthetic photo-like 375 x 500 JPEGs, quality 90, 4:2:0 (tools/jpeg_bench.py's), 100 classes x 16 shots, written to a temporary
folder in the layout `read_folders` reads.  Every figure is the median of `--runs` runs, the candidates alternating:
  build_s            seconds to build the resident train set (read, decode, upload), device decode against DATALOADER.DECODE = "host"
  loader_images_per_s  the train loader alone at B = 256, resident route against streaming route (device decode)
  step_ms            the headline step (ViT-B/16, CoOp-16, 100 classes, B = 256) fed by the resident loader against the same trainer
                     fed by device-resident synthetic batches (what bench.py times), and against it fed the loader's own batches of
                     one epoch, computed beforehand and resident (same pixels, so the operands' values do not enter): the difference
                     to the latter is the input's cost
  describe_aug_ms    host milliseconds per batch of 256 in DeviceTransform.describe_aug, the Python loop that draws the parameters
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.jpeg_bench import encode, synthetic  # noqa: E402


def write_images(root, classes, shots, distinct=256):
    """classes x shots train files (and one test file per class) from `distinct` different synthetic images"""
    blobs = encode(synthetic(distinct), restart=False)
    k = 0
    for split, n in (("train", shots), ("test", 1)):
        for c in range(classes):
            folder = os.path.join(root, split, f"class{c:03d}")
            os.makedirs(folder)
            for j in range(n):
                with open(os.path.join(folder, f"{j:02d}.jpg"), "wb") as f:
                    f.write(blobs[k % distinct])
                k += 1


class Cycling:
    """a loader iterated again and again until `total` batches have been served (a new epoch, a new permutation, each time round)"""

    def __init__(self, loader, total):
        self.loader, self.total = loader, total

    def __len__(self):
        return self.total

    def __iter__(self):
        served = 0
        while served < self.total:
            for batch in self.loader:
                yield batch
                served += 1
                if served == self.total:
                    return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--shots", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--skip-step", action="store_true", help="leave out the training-step comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from mvlpt_amd import class_prompts as CP
    from mvlpt_amd import data as D
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, LookAheadLoader, SyntheticDataManager
    from mvlpt_amd.transforms import build_device_transform
    from mvlpt_amd.weights import ARCHS, make_state_dict
    assert torch.cuda.is_available(), "loader_bench needs a GPU"
    arch = ARCHS[args.arch]
    med = statistics.median

    def sync():
        torch.cuda.synchronize()

    def alternate(candidates):
        """{name: [seconds per run]} of the callables, run alternately, each fenced by a synchronisation"""
        times = {k: [] for k in candidates}
        for _ in range(args.runs):
            for k, fn in candidates.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                times[k].append(time.perf_counter() - t0)
        return times

    def cfg_of(root, resident=16 * 2 ** 30, decode="device"):
        cfg = get_cfg_default()
        cfg.MODEL.BACKBONE.NAME = args.arch
        cfg.INPUT.SIZE = (arch.image_resolution,) * 2
        cfg.DATASET.SOURCES = [["bench", "", root]] if root else []
        cfg.DATASET.NUM_SHOTS = args.shots
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE = args.batch
        cfg.DATALOADER.NUM_WORKERS = 16
        cfg.DATALOADER.RESIDENT_BYTES, cfg.DATALOADER.DECODE = resident, decode
        cfg.TRAINER.MVLPT.COOP.N_CTX = 16
        cfg.TRAIN.PRINT_FREQ, cfg.OPTIM.MAX_EPOCH = 10 ** 9, 10 ** 6
        return cfg

    result = {"classes": args.classes, "shots": args.shots, "batch": args.batch, "runs": args.runs, "image": "375x500 q90 4:2:0 synthetic"}
    with tempfile.TemporaryDirectory() as root:
        write_images(root, args.classes, args.shots)
        cfg = cfg_of(root)
        sd = make_state_dict(arch, seed=1)
        torch.manual_seed(1)
        pre = None
        if CP.BY_CLASS_COUNT.get(args.classes) is not None:      # the class prompts bench.py uses for this class count
            pre, _ = CP.load_class_prompts(CP.BY_CLASS_COUNT[args.classes], 16, cut_contextlen=False, context_length=arch.context_length)
        dm = D.DeviceDataManager(cfg)
        dm.pretokenized = pre
        n_train, W, K = len(dm.train_x), args.warmup, args.steps
        trainer = MVLPT(cfg, dm=dm, clip_state_dict=sd)            # binds the manager: the sets are resident from here on
        loader = dm.train_loader_x
        trainer.train_loader_x = LookAheadLoader(Cycling(loader, W + K + 1), trainer)
        eng, image_set = trainer.model.engine, dm.image_sets["train"]
        result.update(train_images=n_train, resident_bytes=image_set.resident_bytes, n_device=image_set.n_device, n_host=image_set.n_host)

        # (a) building the resident set
        paths, shapes = image_set.paths, image_set.shapes
        t = alternate({d: (lambda d=d: D.ResidentImageSet(eng, paths, shapes, d, 16)) for d in ("device", "host")})
        result["build_s"] = {k: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in t.items()}

        # (b) the loader alone
        stream = D.DeviceLoader(cfg_of(root, resident=0), dm.train_x, train=True)
        stream.bind(eng, None)
        per_epoch = len(loader) * args.batch
        t = alternate({"resident": lambda: [b for b in loader], "streaming": lambda: [b for b in stream]})
        result["loader_images_per_s"] = {k: {"median": round(per_epoch / med(v), 1), "min": round(per_epoch / max(v), 1),
                                             "max": round(per_epoch / min(v), 1)} for k, v in t.items()}
        result["loader_ms_per_batch"] = {k: round(med(v) * 1e3 / len(loader), 3) for k, v in t.items()}

        # (d) the host loop that draws the parameters
        tr = build_device_transform(cfg, eng, train=True, generator=torch.Generator().manual_seed(1))
        batch_shapes = [shapes[i % len(shapes)] for i in range(args.batch)]
        t = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            tr.describe_aug(batch_shapes)
            t.append(time.perf_counter() - t0)
        result["describe_aug_ms"] = {"median": round(med(t) * 1e3, 3), "min": round(min(t) * 1e3, 3), "max": round(max(t) * 1e3, 3),
                                     "transforms": list(cfg.INPUT.TRANSFORMS)}

        # (c) the training step, loader-fed against synthetic-fed
        if not args.skip_step:
            cfg2 = cfg_of("")
            dm2 = SyntheticDataManager(cfg2, args.classes, 4, device="cuda", seed=1234)
            dm2.pretokenized = pre
            torch.manual_seed(1)
            synthetic_fed = MVLPT(cfg2, dm=dm2, clip_state_dict=sd)
            synthetic_fed.train_loader_x = LookAheadLoader(Cycling(dm2.train_loader_x, W + K + 1), synthetic_fed)

            def timed(trn):
                mark = {}

                def hook(i):
                    if i == W:
                        sync()
                        mark["t0"] = time.perf_counter()
                    if i == W + K:
                        sync()
                        mark["t1"] = time.perf_counter()
                        return False
                    return True
                trn.batch_hook = hook
                trn.run_epoch()
                trn.batch_hook = None
                return (mark["t1"] - mark["t0"]) / K
            # ... and against the loader's OWN batches of one epoch, computed beforehand and resident: the same pixels and labels, so
            # that the operands' values (N(0, 1) noise against photographs) do not enter the comparison
            dm3 = SyntheticDataManager(cfg2, args.classes, 1, device="cuda", seed=1234)
            dm3.pretokenized = pre
            dm3.train_loader_x = [b for b in loader]
            torch.manual_seed(1)
            same_fed = MVLPT(cfg2, dm=dm3, clip_state_dict=sd)
            same_fed.train_loader_x = LookAheadLoader(Cycling(dm3.train_loader_x, W + K + 1), same_fed)
            per = {"loader_fed": [], "synthetic_fed": [], "same_batches_resident": []}
            for _ in range(args.runs):
                per["loader_fed"].append(timed(trainer))
                per["synthetic_fed"].append(timed(synthetic_fed))
                per["same_batches_resident"].append(timed(same_fed))
            result["step_ms"] = {k: {"median": round(med(v) * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}
                                 for k, v in per.items()}
            result["step_ms"]["input_cost_ms"] = round((med(per["loader_fed"]) - med(per["synthetic_fed"])) * 1e3, 3)
            result["step_ms"]["input_cost_same_batches_ms"] = round((med(per["loader_fed"]) - med(per["same_batches_resident"])) * 1e3, 3)
            result["step_ms"]["steps_per_run"], result["arch"] = K, args.arch
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
