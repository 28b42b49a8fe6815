#!/usr/bin/env python
"""Headline benchmark: prompt-tuning images/sec (fwd+bwd), ViT-B/16, per-GPU batch 256, synthetic data.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload = BASELINE.json configs[1]: MVLPT with the CoOp head (16 learnable text-context tokens, class token in
the `middle`, 100 classes, text length 77), ViT-B/16, batch 256 per GPU.  One step = `MVLPT.forward_backward`:
image tower forward (no backward is needed: CoOp has no visual prompts), text tower forward +
backward over all 100 class prompts, cosine logits, cross-entropy, prompt-gradient all-reduce, SGD update.
Weak scaling: every rank processes its own 256 images; no data-path collective except the 32 KB gradient
all-reduce.  Prints ONE JSON line on rank 0.

A plain run only sets up, warms up, times the K steps and prints the line (`metric`, `value`, `unit`, `ms_per_step`, ...).
Everything else the line can carry -- CPU baselines, the trim-to-EOT rate, per-kernel / roofline figures, the serialized-tower
pass, all-reduce timing, clock and power, the BASELINE configs[2..4] passes -- runs only with `--full`.
`--dump-outputs DIR` writes what the last timed step handed its caller (loss, accuracy, every prompt parameter after the update
and its gradient) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0   # dense bf16/fp16 MFMA peak of one MI355X (MI355X_MICROARCH.md)
# What a register-only MFMA loop (no LDS, no memory traffic) sustains on pseudo-random fp16 operands: the board throttles to
# ~1.9 GHz at ~1.3 kW (tools/mfma_peak.hip, profiles/r02_power_clock_mfma_only.txt; 2 456 TF/s with constant operands).
# Annotation only: `peak` and `frac` stay on the nominal figure.
MFMA_MEASURED_CEILING_TFLOPS = 1883.0
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "gemm_hbm_traffic.json")   # written from rocprofv3 --pmc passes


def algorithmic_gflop_per_image(arch, B_global, C, L_text, n_ctx, n_vpt, causal_half=True):
    """SURVEY.md §8(d) conventions: 1 MAC = 2 FLOP; frozen weights => no dW; image backward only with visual
    prompts; text tower only with text context, amortised over the global batch, causal attention at half rate."""
    g2 = arch.grid ** 2
    Lv = 1 + n_vpt + g2
    dv, dt = arch.vision_width, arch.transformer_width

    def tower(tokens, L, d, layers, bwd, causal):
        att_f = (2 if causal else 4) * L * d
        att_b = (4 if causal else 8) * L * d
        f = tokens * layers * (24 * d * d + att_f)
        b = tokens * layers * (24 * d * d + att_b) if bwd else 0
        return f + b

    img = tower(Lv, Lv, dv, arch.vision_layers, n_vpt > 0, False)
    img += 2 * g2 * 3 * arch.vision_patch_size ** 2 * dv + 2 * dv * arch.embed_dim
    txt = 0
    if n_ctx > 0:
        txt = C * (tower(L_text, L_text, dt, arch.transformer_layers, True, True) + 2 * dt * arch.embed_dim)
    head = 6 * arch.embed_dim * C
    return (img + head + txt / B_global) / 1e9


def cpu_baseline_images_per_sec(arch, sd, C, L, n_ctx, pre, B_cpu=64, steps=3):
    """Oracle (CPU restatement, kind "port") on the host cores, as BASELINE.md §3 asks: a B = 64 slice of the workload,
    one warm-up step, then >= 3 timed FULL steps (image tower forward, text tower forward + backward over all classes, cosine
    logits, cross-entropy, prompt gradient)."""
    from oracle import clip_oracle as O
    torch.manual_seed(0)
    # thread count: torch defaults to every hardware thread, which is far from the fastest setting on a many-core host
    # (2 x 64-core EPYC: 16 threads run the oracle 4.7x faster than 128) — pick the best of a few counts on a small probe
    probe = torch.randn(4, 3, arch.image_resolution, arch.image_resolution)
    best = None
    for th in sorted({min(c, os.cpu_count() or 1) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(th)
        with torch.no_grad():
            O.image_encoder_fwd(sd, probe[:1], None, None, heads=arch.vision_heads, need_bwd=False)
            t0 = time.perf_counter()
            O.image_encoder_fwd(sd, probe, None, None, heads=arch.vision_heads, need_bwd=False)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, th)
    threads = best[1]
    torch.set_num_threads(threads)
    img = torch.randn(B_cpu, 3, arch.image_resolution, arch.image_resolution)
    layout = O.build_prompt_layout(pre.name_lens, n_ctx, L, "middle")
    eot = pre.tokenized_prompts[:, :L].argmax(dim=-1)
    prefix = torch.randn(C, 1, arch.transformer_width) * 0.02
    suffix = torch.randn(C, L - 1 - n_ctx, arch.transformer_width) * 0.02
    ctx = torch.randn(n_ctx, arch.transformer_width) * 0.02
    label = torch.randint(0, C, (B_cpu,))
    scale = float(sd["logit_scale"].exp())

    def step():
        with torch.no_grad():
            feat, _ = O.image_encoder_fwd(sd, img, None, None, heads=arch.vision_heads, need_bwd=False)
            prompts = O.assemble_prompts(ctx, prefix, suffix, layout)
            txt, tctx = O.text_encoder_fwd(sd, prompts, eot, heads=arch.transformer_heads, need_bwd=True)
            logits, lctx = O.logits_fwd(feat, txt, scale)
            loss, dl = O.cross_entropy_fwd_bwd(logits, label)
            _, dtxt = O.logits_bwd(dl, lctx)
            O.scatter_prompt_grad(O.text_encoder_bwd(sd, dtxt, tctx), layout, tuple(ctx.shape))
        return float(loss)

    t0 = time.perf_counter()
    step()
    t_warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    t = (time.perf_counter() - t0) / steps
    return {"value": round(B_cpu / t, 3), "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": f"oracle/clip_oracle.py (fp32 torch-CPU restatement, pinned by the reference fixtures) on {threads} host "
                      f"threads (fastest of 8/16/32/64 on a probe; the host has {os.cpu_count()} hardware threads): B = {B_cpu} slice of the workload ({C} classes, L = {L}), 1 warm-up step ({t_warm:.1f} s) + "
                      f"{steps} timed full steps of {t:.2f} s (image tower forward, text tower forward+backward, head)"}


class _ClockSampler:
    """Engine clock and board power while the timed region runs, from the amdgpu hwmon files (freq1_input = sclk in Hz,
    power1_input in uW), polled every 50 ms on a host thread.  Under sustained MFMA load the MI355X sits near its 1400 W
    cap and sclk drops from the nominal 2400 MHz (the clock MFMA_PEAK_TFLOPS is quoted at) to 1.7-2.0 GHz: the bench
    line reports the measured clock so that the roofline fraction can also be read against the peak at THAT clock."""
    NOMINAL_MHZ = 2400.0

    def __init__(self):
        import glob
        self.cards = []
        for h in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            if os.path.isfile(h + "/freq1_input") and os.path.isfile(h + "/power1_input"):
                self.cards.append(h)
        self.samples = {h: [] for h in self.cards}
        self._stop, self._thread = False, None

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except (OSError, ValueError):
            return None

    def _run(self):
        while not self._stop:
            for h in self.cards:
                f, p = self._read(h + "/freq1_input"), self._read(h + "/power1_input")
                if f is not None and p is not None:
                    self.samples[h].append((f * 1e-6, p * 1e-6))
            time.sleep(0.05)

    def start(self):
        if self.cards:
            import threading
            self._thread = threading.Thread(target=self._run, daemon=True)
            self._thread.start()

    def stop(self):
        self._stop = True
        if self._thread is not None:
            self._thread.join()
        best = None
        for h, v in self.samples.items():            # several boards may be visible in sysfs: the busy one is ours
            if len(v) >= 2:
                mhz, w = sum(x[0] for x in v) / len(v), sum(x[1] for x in v) / len(v)
                if best is None or w > best["power_w_avg"]:
                    cap = self._read(h + "/power1_cap")
                    best = {"sclk_mhz_avg": round(mhz, 1), "sclk_mhz_min": round(min(x[0] for x in v), 1), "power_w_avg": round(w, 1),
                            "power_cap_w": round(cap * 1e-6, 1) if cap else None, "samples": len(v), "nominal_sclk_mhz": self.NOMINAL_MHZ,
                            "source": "amdgpu hwmon freq1_input / power1_input, 50 ms polling during the timed region"}
        return best


class _CyclingLoader:
    """`total` batches cycling over a few resident synthetic batches (what Dassl's DataLoader is to TrainerX.run_epoch)."""

    def __init__(self, batches, total):
        self.batches, self.total = batches, total

    def __len__(self):
        return self.total

    def __iter__(self):
        for i in range(self.total):
            yield self.batches[i % len(self.batches)]


# BASELINE.json configs[2..4] at their per-GPU shapes on ONE GPU: short fenced passes run AFTER (and outside) the headline's timed
# region, each in its own process of this same script, so that the driver's line carries an observation of every BASELINE
# configuration and not only of configs[1].  cfg4 is listed with CUT_CONTEXTLEN (the reference's multitask
# scripts set TRAINER.CUT_CONTEXTLEN True) — its L = 77 variant is the `tools/config_sweep.sh` line.
SECONDARY_CONFIGS = [
    ("BASELINE configs[2]: MVLPT VPT-deep (8 visual prompt tokens / layer), ViT-B/16, ImageNet-1k class list, per-GPU batch 256",
     ["--method", "vpt", "--classes", "1000", "--batch", "256", "--steps", "6", "--warmup", "2"]),
    ("BASELINE configs[3]: MVLPT UPT (4 text + 4 visual prompts, joint projection), ViT-B/16, 11-dataset class list (2191), per-GPU batch 256, CUT_CONTEXTLEN",
     ["--method", "upt", "--classes", "2191", "--batch", "256", "--cut", "--steps", "4", "--warmup", "2"]),
    ("BASELINE configs[4]: MVLPT UPT, ViT-L/14@336px, ELEVATER-20 class list (1151), per-GPU batch 128",
     ["--arch", "ViT-L/14@336px", "--method", "upt", "--classes", "1151", "--batch", "128", "--steps", "3", "--warmup", "1"]),
]


SECONDARY_BUDGET_S = 300


def run_secondary_configs(dtype):
    import subprocess
    out = []
    t_all = time.perf_counter()
    for workload, flags in SECONDARY_CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--dtype", dtype, "--no-cpu-baseline", "--no-kernel-timing",
               "--no-trim-extra", "--no-secondary"] + flags
        t0 = time.perf_counter()
        entry = {"workload": workload, "flags": " ".join(flags)}
        # bounded: the three children together never add more than SECONDARY_BUDGET_S to the driver's run (a cold box needs ~10 s each)
        left = SECONDARY_BUDGET_S - (t0 - t_all)
        if left < 30:
            entry["skipped"] = f"the {SECONDARY_BUDGET_S} s budget of the secondary passes is used up"
            out.append(entry)
            continue
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=min(200, left), cwd=ROOT)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or len(lines) != 1:
                entry["error"] = (r.stderr or r.stdout)[-400:]
            else:
                j = json.loads(lines[0])
                entry.update({"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "steps": j["steps"], "warmup": j["warmup"],
                              "step_mfma_fraction": j["step_mfma_fraction"], "algorithmic_gflop_per_image": j["algorithmic_gflop_per_image"],
                              "per_gpu_batch": j["config"]["per_gpu_batch"], "child_workload": j["config"]["workload"]})
        except subprocess.TimeoutExpired:
            entry["error"] = "timed out"
        entry["wall_s"] = round(time.perf_counter() - t0, 1)
        out.append(entry)
    return out, round(time.perf_counter() - t_all, 1)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, summary, prompt_learner):
    """What one `MVLPT.forward_backward` hands its caller, from the last timed step: the loss summary, and the prompt
    parameters the step updated with the gradients it computed (`.grad` views of the flat buffer).  fp32 / fp64 .npy files."""
    import numpy as np

    def host(x):
        a = (x.detach().cpu() if torch.is_tensor(x) else torch.tensor(x)).numpy()
        return a.astype(a.dtype if a.dtype == np.float64 else np.float32)

    arrays = {k: host(v) for k, v in summary.items()}
    for name, p in prompt_learner.named_parameters():
        arrays["param." + name] = host(p)
        if p.grad is not None:
            arrays["grad." + name] = host(p.grad)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {DUMP_LIMIT_BYTES})")
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), a)


def _respawn_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: start N ranks ourselves (one process per GPU, RCCL), as the
    reference gets its replicas from one process (nn.DataParallel, trainers/mvlpt.py:877-880)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    import subprocess
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch")
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--method", default="coop", choices=["coop", "vpt", "upt"])
    ap.add_argument("--cut", action="store_true", help="CUT_CONTEXTLEN text length instead of 77")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--trim-eot", action="store_true", help="evaluate the causal text tower only up to max(EOT) (exact; off by default)")
    ap.add_argument("--no-trim-extra", action="store_true", help="skip the extra untimed-for-the-headline pass that reports the --trim-eot rate")
    ap.add_argument("--no-step-pipelining", action="store_true",
                    help="do not compute the next batch's image features underneath the current backward")
    ap.add_argument("--shard-text", dest="shard_text", action="store_true", default=None,
                    help="class-shard the text tower over the ranks; default: on when --gpus > 1 and --classes >= 1000 (the text tower costs "
                         "C * L tokens per step on EVERY rank otherwise), off for small class lists")
    ap.add_argument("--no-shard-text", dest="shard_text", action="store_false", help="replicate the text tower on every rank")
    ap.add_argument("--multitask", action="store_true",
                    help="ELEVATER-style multitask batch: per-task logit mask + soft labels (needs a multitask class list: 2191 / 1151 classes)")
    ap.add_argument("--grad-precision", default="split_grad", choices=["split_grad", "fast"],
                    help="split_grad (default): hi+lo operand pairs (GEMMs and attention) in towers that carry a gradient (prompt "
                         "gradients within 1e-3 of the fp32 CPU path); fast: single 16-bit operands everywhere (~4e-3)")
    ap.add_argument("--text-cus", type=int, default=None,
                    help="compute units of the text tower's partition when the two towers run side by side (CustomCLIP.set_cu_partition; "
                         "0 = shared streams); default: the library's (MVLPT_TEXT_CUS / model.DEFAULT_TEXT_CUS)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short passes of BASELINE configs[2..4] behind the headline run")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--all-kernel-timing", action="store_true", help="bracket every kernel class with marker events (slower)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: CPU baselines, trim-to-EOT pass, per-kernel timing / roofline, "
                         "serialized-tower pass, all-reduce timing, clock sampling, BASELINE configs[2..4] (the --no-* flags above "
                         "switch single legs off again); without it a run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (loss, accuracy, prompt parameters after the update, their gradients) "
                         "as DIR/<name>.npy")
    args = ap.parse_args()
    full = args.full

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _respawn_under_torchrun(args.gpus)

    from mvlpt_amd import class_prompts as CP
    from mvlpt_amd import distributed as D
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    from mvlpt_amd.weights import ARCHS, make_state_dict

    rank, world, local = D.init_process_group()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has {world} rank(s) "
                         f"(launch with torch.distributed.run --nproc-per-node {args.gpus}, or let bench.py spawn them)")
    if world > 1:
        assert torch.distributed.is_initialized() and torch.distributed.get_world_size() == args.gpus
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")

    arch = ARCHS[args.arch]
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = args.arch
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = args.batch
    cfg.TRAINER.MVLPT.COMPUTE_DTYPE = args.dtype
    cfg.TRAINER.MVLPT.GRAD_PRECISION = args.grad_precision
    cfg.TRAINER.MVLPT.STEP_PIPELINING = not args.no_step_pipelining
    cfg.TRAINER.CUT_CONTEXTLEN = args.cut
    cfg.TRAIN.PRINT_FREQ = 10 ** 9          # no host read-back of the loss inside the timed region
    cfg.OPTIM.MAX_EPOCH = 10 ** 6
    n_ctx = n_vpt = 0
    if args.method in ("coop", "upt"):
        n_ctx = 16 if args.method == "coop" else 4
    if args.method in ("vpt", "upt"):
        n_vpt = 8 if args.method == "vpt" else 4
    cfg.TRAINER.MVLPT.COOP.N_CTX, cfg.TRAINER.MVLPT.VPT.N_CTX = n_ctx, n_vpt
    cfg.SEED = 1
    torch.manual_seed(cfg.SEED)      # the prompt initialisation draws from the global generator (train.py: set_random_seed)
    sd = make_state_dict(arch, seed=1)
    # class prompts: the reference tokenizer's own ids for the BASELINE class lists (mvlpt_amd/data/class_prompts.npz)
    list_name = CP.BY_CLASS_COUNT.get(args.classes)
    pre, task_counts, book = None, None, None
    if list_name is not None:
        pre, _ = CP.load_class_prompts(list_name, n_ctx, cut_contextlen=args.cut, context_length=arch.context_length)
        if args.multitask:
            task_counts = CP.task_class_counts(list_name)
            if len(task_counts) < 2:
                raise SystemExit("--multitask needs a multitask class list (--classes 2191 or 1151)")
            book = CP.MultitaskBook.from_list(list_name)      # real task names / class names / label offsets (trainers/mvlpt.py:585-645)
            cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK_LABEL_PERTASK = True
    elif args.multitask:
        raise SystemExit("--multitask needs a multitask class list (--classes 2191 or 1151)")
    n_batches = 4
    W, K = args.warmup, args.steps
    dm = SyntheticDataManager(cfg, args.classes, n_batches, task_class_counts=task_counts, device=dev, seed=1234 + rank,
                              soft_labels=args.multitask, book=book)
    dm.pretokenized = pre
    dm.train_loader_x = _CyclingLoader(dm.train_loader_x, W + K + 1)
    trainer = MVLPT(cfg, dm=dm, clip_state_dict=sd)
    trainer.model.trim_text_to_eot = args.trim_eot
    if args.text_cus is not None:
        trainer.model.set_cu_partition(args.text_cus)
    if args.shard_text is None:
        args.shard_text = world > 1 and args.classes >= 1000 and n_ctx > 0
    if args.shard_text and world > 1:
        trainer.model.enable_class_sharding(rank, world)
    L_text = trainer.model.prompt_learner.tokenized_prompts.shape[1]
    eng = trainer.model.engine
    from mvlpt_amd.engine import device_cus
    eng_cus = device_cus(dev)
    pipeline = cfg.TRAINER.MVLPT.STEP_PIPELINING and n_vpt == 0

    # The timed region is K steps of the trainer's OWN loop (TrainerX.run_epoch, which reads the loader one batch ahead):
    # the hook below brackets steps W .. W+K-1 with barrier + synchronize on both sides.  Every timed step contains
    # exactly one image tower (the prefetch of the following batch), one text tower forward + backward, the head, the
    # gradient all-reduce and the SGD update; the loop is stopped before step W+K runs.
    timing = (full and not args.no_kernel_timing) or args.all_kernel_timing
    sample_every = 1 if args.all_kernel_timing else 4     # dispatch-timestamp timing costs ~2 us per launch: sample steps
    mark = {}

    def fence():
        torch.cuda.synchronize()
        D.barrier()
        torch.cuda.synchronize()

    clk = _ClockSampler() if (rank == 0 and full) else None

    def hook(i):
        if i == W:
            fence()
            if timing:
                eng.profile_begin(all_kernels=args.all_kernel_timing)
            if clk is not None:
                clk.start()
            mark["t0"] = time.perf_counter()
        if i == W + K:
            fence()
            mark["t1"] = time.perf_counter()
            if clk is not None:
                mark["clock"] = clk.stop()
            return False
        if timing and i >= W:
            eng.profile_pause((i - W) % sample_every != 0)
        return True

    trainer.batch_hook = hook
    out = trainer.run_epoch()
    trainer.batch_hook = None
    elapsed = mark["t1"] - mark["t0"]
    stats = eng.profile_end() if timing else {}
    elapsed = D.all_reduce_max(elapsed, dev)
    if args.dump_outputs and rank == 0:      # before any extra pass below moves the prompts on
        dump_outputs(args.dump_outputs, out, trainer.model.prompt_learner)
    # Reported beside the headline, never AS the headline: the same loop with the causal text tower evaluated only up to
    # max(EOT) (positions after EOT can reach neither a logit nor a gradient; exact, tests/test_hip_model.py::
    # test_trim_to_eot_is_exact).  `value` keeps all L positions, as the reference computes them.
    trim_line = None
    if full and n_ctx and not args.trim_eot and not args.cut and not args.no_trim_extra and K >= 8:
        trainer.model.trim_text_to_eot = True
        W2, K2 = 4, min(K, 16)
        dm.train_loader_x = _CyclingLoader(dm.train_loader_x.batches, W2 + K2 + 1)
        trainer.train_loader_x = dm.train_loader_x
        mark2 = {}

        def hook2(i):
            if i == W2:
                fence()
                mark2["t0"] = time.perf_counter()
            if i == W2 + K2:
                fence()
                mark2["t1"] = time.perf_counter()
                return False
            return True

        trainer.batch_hook = hook2
        trainer.run_epoch()
        trainer.batch_hook = None
        e2 = D.all_reduce_max(mark2["t1"] - mark2["t0"], dev)
        trainer.model.trim_text_to_eot = False
        trim_line = {"value": round(args.batch * world * K2 / e2, 2), "ms_per_step": round(1e3 * e2 / K2, 3), "steps": K2,
                     "text_positions_evaluated": int(trainer.model.prompt_learner.max_eot + 1),
                     "note": "same loop, causal text tower evaluated up to max(EOT) only (exact: later positions reach no logit and no gradient); not the headline"}
    # Untimed extra pass: the same step with the two towers serialized on one stream and no cross-step prefetch, so each
    # GEMM launch has the chip to itself.  In the timed region the text tower runs on a second stream underneath the
    # image tower; concurrent kernels stretch each other's durations, which inflates per-launch times (they then sum
    # to more than the step) without being slower overall.  Reported next to the timed-region figure.
    stats_serial = {}
    if timing and trainer.model.overlap_towers:      # every rank takes part (the step contains the gradient all-reduce)
        trainer.model.overlap_towers = False
        cfg.TRAINER.MVLPT.STEP_PIPELINING = False
        batches = dm.train_loader_x.batches
        trainer.forward_backward(batches[0])
        torch.cuda.synchronize()
        eng.profile_begin(all_kernels=False)
        for i in range(3):
            trainer.forward_backward(batches[i % n_batches])
        torch.cuda.synchronize()
        stats_serial = eng.profile_end()
        trainer.model.overlap_towers = True
    loss = float(out["loss"])
    assert loss == loss, "loss is NaN"

    from mvlpt_amd import _lib as _L
    import re as _re
    lib_version = _L.lib.mvlpt_version().decode()
    lib_src_hash = (_re.search(r"src:(\w+)", lib_version) or [None, None])[1]
    # N > 1: who took part.  Every rank reports its device; the line shows N distinct devices on the RCCL backend without anyone
    # reading logs, and the flat gradient all-reduce timed by itself (events, 20 calls after the timed region).
    ranks_info, allreduce_us = None, None
    shared_gpu_debug = os.environ.get("MVLPT_DEBUG_SHARE_GPU", "0") == "1"
    if world > 1:
        prop = torch.cuda.get_device_properties(local)
        mine = {"rank": rank, "local_device": local, "device_name": prop.name, "device_uuid": str(getattr(prop, "uuid", "")),
                "pci_bus_id": getattr(prop, "pci_bus_id", None), "backend": torch.distributed.get_backend(), "pid": os.getpid(),
                "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES")}
        ranks_info = [None] * world
        torch.distributed.all_gather_object(ranks_info, mine)
        flats = [f.flat for f in getattr(trainer, "_flat_grads", {}).values() if f.flat.numel()]
        if full and flats and not shared_gpu_debug:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            scratch = flats[0].clone()
            for _ in range(3):
                torch.distributed.all_reduce(scratch, op=torch.distributed.ReduceOp.AVG)
            fence()
            e0.record()
            for _ in range(20):
                torch.distributed.all_reduce(scratch, op=torch.distributed.ReduceOp.AVG)
            e1.record()
            torch.cuda.synchronize()
            allreduce_us = {"value": round(e0.elapsed_time(e1) * 1e3 / 20, 1), "bytes": int(scratch.numel() * scratch.element_size()),
                            "calls": 20, "note": "the step's one collective (flat fp32 prompt-gradient buffer, in-place AVG), back to back, event-timed on rank 0"}
    if rank == 0:
        B_global = args.batch * world
        ips = B_global * K / elapsed
        L_alg = (trainer.model.prompt_learner.max_eot + 1) if args.trim_eot else L_text   # charge only evaluated positions
        gf_img = algorithmic_gflop_per_image(arch, B_global, args.classes, L_alg, n_ctx, n_vpt)
        is_headline = (args.method, args.arch, args.classes, args.batch, args.cut, args.multitask) == ("coop", "ViT-B/16", 100, 256, False, False)
        line = {
            "metric": "prompt-tuning images/sec (fwd+bwd), ViT-B/16 bs=256, 1/2/4/8 MI355X",
            "value": round(ips, 2), "unit": "images/sec", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": round(1e3 * elapsed / K, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": (("BASELINE configs[1]: " if is_headline else "variant: ") +
                                    f"MVLPT {args.method} head, {args.arch}, {args.classes} classes"
                                    f"{' (' + list_name + ' token table)' if list_name else ' (synthetic token ids)'}, "
                                    f"n_ctx={n_ctx} n_vpt={n_vpt}, text L={L_text}, class token middle"
                                    f"{', per-task mask + soft labels' if args.multitask else ''}"),
                       "text_positions_evaluated": (trainer.model.prompt_learner.max_eot + 1) if args.trim_eot else L_text,
                       "loop": "TrainerX.run_epoch = the plain Dassl loop `for batch in train_loader_x: forward_backward(batch)`; the one-batch look-ahead comes from the loader (LookAheadLoader, installed by MVLPT.build_data_loader)", "step_pipelining": bool(pipeline),
                       "grad_precision": args.grad_precision,
                       "layernorm_folding": {"0": "off", "1": "image tower", "2": "both towers"}.get(os.environ.get("MVLPT_LN_FOLD", "2"), "both towers"),
                       "residual_stream": "packed fp16 + byte (image tower without prompts / backward)" if (os.environ.get("MVLPT_RESID_PACKED", "1") not in ("", "0") and n_vpt == 0 and args.dtype == "fp16") else "fp32",
                       "cu_partition": ({"text_tower_cus": trainer.model.text_cus, "image_tower_cus": eng_cus - trainer.model.text_cus}
                                        if trainer.model.text_cus else "none (towers share every compute unit)"),
                       "per_gpu_batch": args.batch, "global_batch": B_global, "parallelism": f"dp{world}",
                       "text_tower": "class-sharded over ranks" if (args.shard_text and world > 1) else "replicated per GPU", "loss": round(loss, 5)},
            "step_mfma_fraction": round(ips / world * gf_img / (MFMA_PEAK_TFLOPS * 1e3), 4),
            "algorithmic_gflop_per_image": round(gf_img, 3),
            "library": lib_version,
        }
        if ranks_info is not None:
            ids = {(r.get("device_uuid") or "", str(r.get("pci_bus_id")), r["local_device"]) for r in ranks_info}
            line["config"]["ranks"] = ranks_info
            line["config"]["distinct_devices"] = len(ids)
            if shared_gpu_debug:
                line["config"]["debug_shared_gpu"] = "MVLPT_DEBUG_SHARE_GPU=1: every rank on cuda:0, collectives through gloo (a test mode, not a measurement)"
            else:
                assert len(ids) == world, f"{world} ranks but {len(ids)} distinct devices: {ranks_info}"
                assert all(r["backend"] == "nccl" for r in ranks_info), "N > 1 must run on RCCL (backend nccl)"
            line["allreduce_us"] = allreduce_us
        clock = mark.get("clock")
        if clock:
            line["clock"] = clock
            sustained = MFMA_PEAK_TFLOPS * clock["sclk_mhz_avg"] / _ClockSampler.NOMINAL_MHZ
            line["step_mfma_fraction_at_measured_clock"] = round(ips / world * gf_img / (sustained * 1e3), 4)
        traffic = None
        # offline PMC passes (tools/r03_profile.sh): the headline's file, and one per BASELINE config that carries an image backward
        cfg_key = {("vpt", "ViT-B/16", 1000): "cfg3", ("upt", "ViT-B/16", 2191): "cfg4", ("upt", "ViT-L/14@336px", 1151): "cfg5"}.get(
            (args.method, args.arch, args.classes))
        tfile = TRAFFIC_FILE if is_headline else (TRAFFIC_FILE.replace(".json", f"_{cfg_key}.json") if cfg_key and not args.cut else None)
        traffic_note = None
        if tfile and os.path.isfile(tfile):
            with open(tfile) as f:
                traffic = json.load(f)       # {"bytes_per_launch": …, "source": "rocprofv3 --pmc …", "lib_src_hash": …}
            # the PMC passes are offline: the figure only describes THIS run if it was taken on the binary that is loaded now
            if traffic.get("lib_src_hash") != lib_src_hash:
                traffic_note = (f"{os.path.relpath(tfile, ROOT)} was recorded on library src:{traffic.get('lib_src_hash')} but the loaded "
                                f"library is src:{lib_src_hash}: dropped (re-record with tools/r06_profile.sh)")
                traffic = None
        n_sampled = len(range(0, K, sample_every))
        if "gemm_bt" in stats:
            g = stats["gemm_bt"]
            # achieved = algorithmic FLOPs of the launches / time during which the kernel occupies the GPU.  The text
            # tower's GEMMs run on a second stream underneath the image tower's, so launch intervals overlap: the
            # occupied time is the UNION of the intervals (dispatch timestamps), not the sum of durations (which
            # would count concurrent stretches twice).  Both are reported; they coincide when nothing overlaps.
            tf = g["flops"] / (g["busy_ms"] * 1e-3) / 1e12
            tf_sum = g["flops"] / (g["ms"] * 1e-3) / 1e12
            line["roofline"] = {"bound": "mfma", "kernel": "gemm_bt_kernel + gemm_pc_kernel + gemm_pcp_kernel (all epilogues)", "achieved": round(tf, 1),
                                "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / MFMA_PEAK_TFLOPS, 4),
                                "traffic": traffic, "launches_per_step": g["launches"] // n_sampled, "steps_sampled": n_sampled,
                                "avg_launch_us": round(1e3 * g["ms"] / g["launches"], 2),
                                "busy_us_per_launch": round(1e3 * g["busy_ms"] / g["launches"], 2),
                                "achieved_sum_of_durations": round(tf_sum, 1),
                                "executed_over_algorithmic_flops": round(g["flops_executed"] / g["flops"], 4),
                                "achieved_executed": round(g["flops_executed"] / (g["busy_ms"] * 1e-3) / 1e12, 1),
                                "algorithmic_bytes_per_launch": int(g["bytes"] / g["launches"]),
                                "concurrency": "timed region: text tower on a 2nd stream and the next batch's image tower on a 3rd overlap; achieved = FLOPs / union of the launch intervals",
                                "note": "achieved / frac charge ALGORITHMIC FLOPs (2MNK per linear); launches with split-precision operands execute twice that (achieved_executed)"}
            line["roofline"]["measured_mfma_only_ceiling"] = {"value": MFMA_MEASURED_CEILING_TFLOPS, "unit": "TFLOP/s",
                                                              "frac": round(tf / MFMA_MEASURED_CEILING_TFLOPS, 4),
                                                              "source": "profiles/r02_power_clock_mfma_only.txt (register-only MFMA loop, pseudo-random fp16 operands, 1.9 GHz at 1.3 kW)"}
            if traffic_note:
                line["roofline"]["traffic_note"] = traffic_note
            # the launches of the dominant kernel once more per problem: the four GEMMs of an image-tower block by name, then the rest
            # by total time.  frac = 2MNK / average launch duration / peak, from the same dispatch timestamps as `achieved`.
            Ti = args.batch * (1 + n_vpt + arch.grid ** 2)
            dvw = arch.vision_width
            names = {(Ti, 3 * dvw, dvw): "image QKV", (Ti, dvw, dvw): "image out-projection", (Ti, 4 * dvw, dvw): "image MLP up + GELU",
                     (Ti, dvw, 4 * dvw): "image MLP down"}
            per_kernel = []
            for k, v in stats.items():
                m = _re.match(r"g(\d+)x(\d+)x(\d+) e(\d+) s(\d+) f(\d+)$", k)
                if not m:
                    continue
                Mq, Nq, Kq, eq, sq, fq = (int(x) for x in m.groups())
                avg_us = 1e3 * v["ms"] / v["launches"]
                epi_names = {0: "store16", 1: "gelu", 2: "resid32", 3: "gelu_bwd", 4: "store32", 5: "gelu_split", 6: "gelu_bwd_split", 7: "store_split",
                             8: "resid32 + LayerNorm producer", 13: "packed residual + LayerNorm producer"}
                per_kernel.append({"name": names.get((Mq, Nq, Kq), "text tower / head" if Mq != Ti else "image tower, other"), "M": Mq, "N": Nq, "K": Kq,
                                   "epilogue": epi_names.get(eq, str(eq)),
                                   "operands": {0: "single", 1: "16-bit pair", 2: "mixed pair"}[sq], "ln_fold_consumer": bool(fq),
                                   "launches_per_step": round(v["launches"] / n_sampled, 2), "avg_us": round(avg_us, 1),
                                   "tflops": round(2.0 * Mq * Nq * Kq / avg_us / 1e6, 1),
                                   "frac": round(2.0 * Mq * Nq * Kq / (avg_us * 1e-6) / (MFMA_PEAK_TFLOPS * 1e12), 4)})
            per_kernel.sort(key=lambda r: -r["avg_us"] * r["launches_per_step"])
            line["roofline"]["per_kernel"] = per_kernel[:12]
            if "attention_fwd_image" in stats:
                a = stats["attention_fwd_image"]
                au = 1e3 * a["ms"] / a["launches"]
                line["roofline"]["image_attention_fwd"] = {"launches_per_step": round(a["launches"] / n_sampled, 2), "avg_us": round(au, 1),
                                                           "algorithmic_bytes": int(a["bytes"] / a["launches"]),
                                                           "gb_per_s": round(a["bytes"] / a["launches"] / au / 1e3, 1),
                                                           "frac_of_hbm_8tbs": round(a["bytes"] / a["launches"] / (au * 1e-6) / 8e12, 4),
                                                           "mfma_frac": round(a["flops"] / a["launches"] / (au * 1e-6) / (MFMA_PEAK_TFLOPS * 1e12), 4)}
            if clock:
                line["roofline"]["peak_at_measured_clock"] = round(sustained, 1)
                line["roofline"]["frac_at_measured_clock"] = round(tf / sustained, 4)
            if "gemm_bt" in stats_serial:
                gs = stats_serial["gemm_bt"]
                tfs = gs["flops"] / (gs["ms"] * 1e-3) / 1e12
                line["roofline"]["serialized_towers"] = {"achieved": round(tfs, 1), "frac": round(tfs / MFMA_PEAK_TFLOPS, 4),
                                                         "achieved_executed": round(gs["flops_executed"] / (gs["ms"] * 1e-3) / 1e12, 1),
                                                         "avg_launch_us": round(1e3 * gs["ms"] / gs["launches"], 2),
                                                         "note": "3 untimed steps, everything on one stream, no cross-step prefetch"}
            # (three streams overlap in the timed region and concurrent kernels stretch each other: these are SUMS of
            # per-launch durations per kernel class, not shares of the step, and may add up to more than ms_per_step)
            line["kernel_duration_sums_ms_per_step"] = {k: round(v["ms"] / n_sampled, 3) for k, v in stats.items()}
            line["kernel_duration_sums_ms_per_step"]["note"] = "sum of launch durations under 3 overlapping streams; can exceed ms_per_step"
            # executed (not algorithmic) step-level fraction: GEMM FLOPs actually issued per step (CLS-only / EOT-only last
            # blocks skip work the reference computes and never reads; split-precision GEMMs issue twice their 2MNK)
            # plus the attention FLOPs at their algorithmic count
            att = (args.batch * arch.vision_layers * 4 * (1 + n_vpt + arch.grid ** 2) ** 2 * arch.vision_width * (3 if n_vpt else 1)
                   + (args.classes * arch.transformer_layers * 2 * L_text ** 2 * arch.transformer_width * 3 if n_ctx else 0))
            line["step_mfma_fraction_executed"] = round((g["flops_executed"] / n_sampled + att) / (elapsed / K) / (MFMA_PEAK_TFLOPS * 1e12), 4)
        if trim_line is not None:
            line["text_trimmed_to_eot"] = trim_line
        if full and world == 1 and not args.no_cpu_baseline and args.method == "coop" and pre is not None:
            line["cpu_baseline"] = cpu_baseline_images_per_sec(arch, sd, args.classes, L_text, n_ctx, pre)
            if is_headline:
                # configs[0], the reference's own CPU-runnable case (ViT-B/32, B = 32, same class list)
                from mvlpt_amd.weights import ARCHS as _A, make_state_dict as _mk
                a32 = _A["ViT-B/32"]
                line["cpu_baseline_cfg1"] = cpu_baseline_images_per_sec(a32, _mk(a32, seed=cfg.SEED), args.classes, L_text, n_ctx, pre, B_cpu=32)
                line["cpu_baseline_cfg1"]["config"] = "BASELINE configs[0]: CoOp ViT-B/32, 100 classes, n_ctx=16, L=77, full batch of 32"
        if full and is_headline and world == 1 and not args.no_secondary and args.grad_precision == "split_grad":
            # this process is done with the GPU (everything above is synchronised): the children have it to themselves
            del trainer, dm
            torch.cuda.empty_cache()
            line["secondary_configs"], line["secondary_configs_wall_s"] = run_secondary_configs(args.dtype)
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
