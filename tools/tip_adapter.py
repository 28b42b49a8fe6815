"""Tip-Adapter / Tip-Adapter-F on saved features, with the cache head on the device:

    python tools/tip_adapter.py --dataset Caltech101 --feature_dir clip_feat --text_features clip_feat/Caltech101/text.npz

reads `{feature_dir}/{dataset}/{train,val,test}.npz` (keys feature_list / label_list: the files tools/linear_probe.py reads, written by
mvlpt_amd.linear_probe.save_split) and the text features of the class prompts (`feature_list` [n_cls, D], normalised here).  The train
split is the few-shot set: its rows are the cache keys (one pass, no augmentation: the images are not here).  (beta, alpha) are
searched on val with the published 200 x 20 grid; --finetune runs Tip-Adapter-F on the train rows first.  Prints the zero-shot, the
Tip-Adapter and the searched accuracy on test.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Rows:
    """A feature split as the (images, labels) batches TipAdapterHead.fit takes: the "images" are the saved features."""

    def __init__(self, features, labels, batch_size):
        self.f, self.y, self.b = features, labels, batch_size

    def __len__(self):
        return (len(self.y) + self.b - 1) // self.b

    def __iter__(self):
        for i in range(0, len(self.y), self.b):
            yield self.f[i:i + self.b], self.y[i:i + self.b]


class _Identity:
    """Stands where the frozen CLIP goes: the rows are features already."""

    @staticmethod
    def encode_image(x):
        return x


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", type=str, default="", help="sub-directory of feature_dir")
    ap.add_argument("--feature_dir", type=str, default="clip_feat", help="feature dir path")
    ap.add_argument("--text_features", type=str, required=True, help="npz with feature_list [n_cls, D]: the class prompts' text features")
    ap.add_argument("--logit_scale", type=float, default=100.0, help="exp(logit_scale) of the CLIP the features come from")
    ap.add_argument("--init_alpha", type=float, default=1.0)
    ap.add_argument("--init_beta", type=float, default=5.5)
    ap.add_argument("--finetune", action="store_true", help="Tip-Adapter-F: fine-tune the cache keys on the train rows")
    ap.add_argument("--train_epoch", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--eps", type=float, default=1e-4)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from mvlpt_amd import linear_probe as LP
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.tip_adapter import TipAdapterHead
    from mvlpt_amd.weights import ARCHS

    dev = torch.device("cuda")
    path = os.path.join(args.feature_dir, args.dataset)
    (train_f, train_y), (val_f, val_y), (test_f, test_y) = [LP.load_split(path, s) for s in ("train", "val", "test")]
    with np.load(args.text_features) as f:
        text = torch.from_numpy(np.asarray(f["feature_list"], np.float32)).to(dev)
    engine = Engine(ARCHS["tiny"], device=dev)        # the head's entries are handle-free: any engine serves
    text = engine.text_ensemble(text.view(1, *text.shape))
    head = TipAdapterHead(engine, text, args.logit_scale, alpha=args.init_alpha, beta=args.init_beta)
    head.from_features(train_f, train_y, text.shape[0])

    def accuracy(h):
        return h.accuracy(test_f, test_y)

    saved = head.alpha
    head.alpha = 0.0
    print(f"zero-shot CLIP: {accuracy(head):.2f}", flush=True)
    head.alpha = saved
    print(f"Tip-Adapter (alpha {head.alpha}, beta {head.beta}): {accuracy(head):.2f}", flush=True)
    if args.finetune:
        tf, ty = torch.from_numpy(np.asarray(train_f, np.float32)).to(dev), torch.from_numpy(np.asarray(train_y, np.int64)).to(dev)
        head.fit(_Identity, lambda: _Rows(tf, ty, args.batch_size), args.train_epoch, args.lr, args.eps, eval_set=(val_f, val_y))
        for epoch, loss, acc, held in head.history:
            print(f"epoch {epoch + 1}: loss {loss:.4f} train {acc:.2f} val {held:.2f}", flush=True)
        print(f"Tip-Adapter-F: {accuracy(head):.2f}", flush=True)
    beta, alpha, val_acc, _ = head.search_hp(val_f, val_y)
    print(f"search on val: beta {beta:.4f} alpha {alpha:.4f} val {val_acc:.2f}; test {accuracy(head):.2f}", flush=True)
    engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
