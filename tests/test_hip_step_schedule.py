"""The schedule of a training step, call for call (-m gpu): which engine entry is enqueued on which stream, and every wait, event and
record_stream between the streams.

The schedule lives in mvlpt_amd/schedule.py (DESIGN.md "Step schedule").  tests/golden/step_schedule.json was recorded by
tools/make_step_schedule_golden.py from the Python tree in front of that module, on the same library, so the test holds the module to
the schedule it replaced: per scenario the log of calls, the sha256 of every step's loss and of every prompt parameter after the last
step must be EQUAL (nothing reorders a sum).  The recorder therefore touches only names both trees have: the `Engine` entries,
`mvlpt_amd.engine.set_stream_cu_cap`, the trainer's `parse_batch_train`, and torch's own stream / event methods.

Streams and events are numbered by first appearance within a scenario (stream 0 is the one the scenario starts on)."""
import contextlib
import hashlib
import inspect
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_schedule.json")

ENGINE_CALLS = ("image_fwd", "image_fwd_begin", "image_fwd_resume", "image_fwd_abandon", "image_bwd",
                "text_fwd", "text_fwd_deep", "text_fwd_ranged", "text_bwd", "text_bwd_deep",
                "logits_fwd", "logits_bwd", "logits_ranged_fwd", "logits_ranged_bwd", "cross_entropy", "set_vpt_dropout")
LOGGED_ARGUMENTS = ("save_for_bwd", "stop_block", "need_img", "need_txt")


class Recorder:
    """Logs the calls of one scenario.  `with Recorder() as rec:` wraps the classes, `rec.trainer(tr)` one trainer's
    parse_batch_train and forward_backward; everything is restored on exit."""

    def __init__(self):
        self.log, self.losses = [], []
        self._streams, self._events, self._seen_events = {}, {}, []
        self._nested = 0               # inside Stream.wait_stream: the record_event / wait_event it is made of are not logged
        self._restore = []

    # -- numbering
    def stream(self, s=None) -> int:
        s = torch.cuda.current_stream() if s is None else s
        return self._streams.setdefault((s.device.index, s.cuda_stream), len(self._streams))

    def event(self, e) -> int:
        if id(e) not in self._events:
            self._events[id(e)] = len(self._events)
            self._seen_events.append(e)      # kept alive: no id is reused within the scenario
        return self._events[id(e)]

    # -- wrapping
    def _wrap(self, owner, name, make):
        had = name in vars(owner)            # else inherited (Tensor.record_stream, a trainer's bound methods): removed again on exit
        orig = vars(owner)[name] if had else getattr(owner, name)
        self._restore.append((owner, name, orig, had))
        setattr(owner, name, make(orig))

    def _engine_call(self, name):
        def make(orig):
            sig = inspect.signature(orig)

            def wrapped(eng, *a, **k):
                given = sig.bind(eng, *a, **k).arguments
                entry = [name, self.stream()]
                extra = {n: int(given[n]) for n in LOGGED_ARGUMENTS if n in given}
                if name == "set_vpt_dropout":
                    extra["masks"] = given["masks"] is not None
                self.log.append(entry + ([extra] if extra else []))
                return orig(eng, *a, **k)
            return wrapped
        return make

    def __enter__(self):
        from mvlpt_amd import engine as E
        self.stream()                        # stream 0: where the scenario starts
        try:
            for name in ENGINE_CALLS:
                self._wrap(E.Engine, name, self._engine_call(name))
            self._wrap(E, "set_stream_cu_cap", lambda orig: lambda st, n: (
                self.log.append(["set_stream_cu_cap", self.stream(), self.stream(st), int(n)]), orig(st, n))[1])

            def wait_stream(orig):
                def wrapped(s, other):
                    self.log.append(["wait_stream", self.stream(s), self.stream(other)])
                    self._nested += 1
                    try:
                        return orig(s, other)
                    finally:
                        self._nested -= 1
                return wrapped

            def wait_event(orig):
                def wrapped(s, ev):
                    if not self._nested:
                        self.log.append(["wait_event", self.stream(s), self.event(ev)])
                    return orig(s, ev)
                return wrapped

            def record(orig):
                def wrapped(ev, stream=None):
                    if not self._nested:
                        self.log.append(["event_record", self.event(ev), self.stream(stream)])
                    return orig(ev) if stream is None else orig(ev, stream)
                return wrapped

            def record_stream(orig):
                def wrapped(t, s):
                    self.log.append(["record_stream", list(t.shape), self.stream(s)])
                    return orig(t, s)
                return wrapped

            self._wrap(torch.cuda.Stream, "wait_stream", wait_stream)
            self._wrap(torch.cuda.Stream, "wait_event", wait_event)
            self._wrap(torch.cuda.Event, "record", record)
            self._wrap(torch.Tensor, "record_stream", record_stream)
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        for owner, name, orig, had in reversed(self._restore):
            if had:
                setattr(owner, name, orig)
            else:
                delattr(owner, name)
        self._restore = []
        return False

    def trainer(self, tr):
        """Log `tr.parse_batch_train` with the batch's position in the train loader, keep every step's loss."""
        batches = list(tr.dm.train_loader_x)

        def parse(orig):
            def wrapped(batch):
                self.log.append(["parse_batch_train", [i for i, b in enumerate(batches) if b is batch][0]])
                return orig(batch)
            return wrapped

        def step(orig):
            def wrapped(batch):
                out = orig(batch)
                self.losses.append(out["loss"])
                return out
            return wrapped
        self._wrap(tr, "parse_batch_train", parse)
        self._wrap(tr, "forward_backward", step)
        return tr

    def result(self, tr):
        torch.cuda.synchronize()
        digest = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        return {"log": self.log, "losses": [digest(x) for x in self.losses],
                "params": {k: digest(v) for k, v in tr.model.prompt_learner.named_parameters()}}


@contextlib.contextmanager
def cfg_defaults(*settings):
    """`make_trainer` builds its model from get_cfg_default(): settings it has no argument for go in as defaults, as a
    merge_from_list list."""
    from mvlpt_amd import config
    orig = config.get_cfg_default

    def patched():
        cfg = orig()
        cfg.merge_from_list([str(s) for s in settings])
        return cfg
    config.get_cfg_default = patched
    try:
        yield
    finally:
        config.get_cfg_default = orig


def _coop(tmp_path, rec, method="coop", setup=None, settings=(), **kw):
    from tests.test_hip_trainer import make_trainer
    torch.manual_seed(0)
    with cfg_defaults(*settings):
        tr = make_trainer(tmp_path, method, **kw)
    tr.cfg.TRAIN.PRINT_FREQ = 10 ** 9
    if setup is not None:
        setup(tr)
    return rec.trainer(tr)


def _epoch(**kw):
    def run(tmp_path, rec):
        tr = _coop(tmp_path, rec, **kw)
        tr.run_epoch()
        return tr
    return run


def _set(**attrs):
    def setup(tr):
        for k, v in attrs.items():
            setattr(tr.model, k, v)
    return setup


def _pipelining_off(tr):
    tr.cfg.TRAINER.MVLPT.STEP_PIPELINING = False      # as bench.py toggles it: the loader still reads ahead


def _eval_train_eval(tmp_path, rec):
    tr = _coop(tmp_path, rec)
    tr.test()
    tr.test()
    tr.set_model_mode("train")
    tr.num_batches, tr.batch_idx = 10, 0
    tr.forward_backward(tr.dm.train_loader_x[0])
    tr.test()
    return tr


def _leave_early(split):
    def run(tmp_path, rec):
        tr = _coop(tmp_path, rec, setup=_set(prefetch_split=split))
        # two steps bring the split schedule to the point where a tower is begun (the first step has no features to pick up);
        # without the split one step already leaves a whole prefetched tower behind
        stop_after = 1 if split[0] else 0
        tr.batch_hook = lambda i: i <= stop_after
        tr.run_epoch()
        tr.batch_hook = None
        tr.run_epoch()
        return tr
    return run


def _begun_and_given_up(tmp_path, rec):
    """A tower begun for the next batch that nobody resumes: the epilogue gives it up; the next epoch starts clean."""
    tr = _coop(tmp_path, rec, setup=_set(prefetch_split=(1, 8)))
    tr.set_model_mode("train")
    tr.num_batches = 4
    it = iter(tr.train_loader_x)
    tr.batch_idx = 0
    tr.forward_backward(next(it))
    image = tr.parse_batch_train(tr.dm.train_loader_x[2])[0]
    tr.model.prefetch_image_features(image, stop_block=1, cu_cap=8)
    it.close()
    tr.end_of_epoch_loop()
    tr.run_epoch()
    return tr


def _mvlpt_cocoop(vpt):
    def run(tmp_path, rec):
        from tests.test_hip_mvlpt_cocoop import _trainer
        torch.manual_seed(0)
        tr, dm = _trainer(tmp_path, vpt)
        rec.trainer(tr)
        tr.num_batches, tr.batch_idx = 100, 0
        for _ in range(2):
            tr.forward_backward(dm.train_loader_x[0])
        return tr
    return run


def _cocoop(tmp_path, rec):
    from tests.test_hip_cocoop import _trainer
    torch.manual_seed(0)
    tr, dm = _trainer(tmp_path)
    rec.trainer(tr)
    tr.num_batches, tr.batch_idx = 100, 0
    for _ in range(2):
        tr.forward_backward(dm.train_loader_x[0])
    return tr


# name -> run(tmp_path, recorder) -> the trainer.  make_trainer's tower ("tiny") and its 4 batches of 8 images throughout.
SCENARIOS = {
    "coop": _epoch(),
    "coop_prefetch_split": _epoch(setup=_set(prefetch_split=(1, 8))),
    "coop_step_pipelining_off": _epoch(setup=_pipelining_off),
    "coop_towers_on_one_stream": _epoch(setup=_set(overlap_towers=False)),
    "coop_cu_partition": _epoch(setup=lambda tr: tr.model.set_cu_partition(64)),
    "vpt": _epoch(method="vpt"),
    "upt": _epoch(method="upt"),
    "coop_multitask_pertask_labels": _epoch(tasks=[2, 1, 3]),
    "vpt_constant_text_features": _epoch(method="vpt", settings=("TRAINER.MVLPT.COOP.N_CTX", 0)),
    "coop_deep_text": _epoch(settings=("TRAINER.MVLPT.COOP.N_DEEP", 1)),
    "test_test_step_test": _eval_train_eval,
    "leave_after_first_step_then_epoch": _leave_early((0, 0)),
    "leave_with_split_then_epoch": _leave_early((1, 8)),
    "begun_tower_given_up_then_epoch": _begun_and_given_up,
    "mvlpt_cocoop_two_steps": _mvlpt_cocoop(0),
    "mvlpt_cocoop_vpt_two_steps": _mvlpt_cocoop(2),
    "cocoop_two_steps": _cocoop,
}


def record(name, tmp_path):
    with Recorder() as rec:
        tr = SCENARIOS[name](tmp_path, rec)
        return rec.result(tr)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_the_scenarios(golden):
    assert set(golden) == set(SCENARIOS)
    # the scenarios reach what they are there for
    calls = lambda name: [e[0] for e in golden[name]["log"]]
    assert "image_fwd_begin" in calls("coop_prefetch_split") and "image_fwd_resume" in calls("coop_prefetch_split")
    assert "image_fwd_abandon" in calls("begun_tower_given_up_then_epoch")
    assert "text_fwd_deep" in calls("coop_deep_text") and "text_bwd_deep" in calls("coop_deep_text")
    assert calls("vpt_constant_text_features").count("text_fwd") == 1 and calls("test_test_step_test").count("text_fwd") == 3
    assert "text_fwd_ranged" in calls("mvlpt_cocoop_two_steps") and "image_bwd" in calls("mvlpt_cocoop_vpt_two_steps")
    assert {e[1] for e in golden["coop_cu_partition"]["log"] if e[0] == "text_bwd"} == {1}       # the backward on the text stream
    assert {e[1] for e in golden["coop_towers_on_one_stream"]["log"] if e[0] == "text_fwd"} == {0}
    assert {e[1] for e in golden["coop"]["log"] if e[0] == "text_fwd"} == {1}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_schedule_is_the_recorded_one(golden, tmp_path, name):
    got, want = record(name, tmp_path), golden[name]
    for i, (g, w) in enumerate(zip(got["log"], want["log"])):
        assert g == w, f"{name}: call {i} is {g}, recorded {w}; before it: {got['log'][max(0, i - 6):i]}"
    assert len(got["log"]) == len(want["log"]), f"{name}: {len(got['log'])} calls, recorded {len(want['log'])}"
    assert got["losses"] == want["losses"] and len(got["losses"]) > 0, f"{name}: a step's loss differs in its bits"
    assert got["params"] == want["params"], f"{name}: a prompt parameter differs in its bits"
