"""What the engine remembers of a forward (-m gpu): call sequences on the C entries and what each call answers.

The engine keeps one record per job (image tower, text tower, head) with one phase each (csrc/engine.hip `Phase`, DESIGN.md "Engine
state").  A sequence is a list of calls; its expectation is every call's return code and, for a refusal, the text of mvlpt_last_error.
The calls go straight to `_lib.lib`: the Python `Engine` mirrors some of this state and refuses several of these sequences before C
sees them.

RECORDED sequences are expected to answer what the library answered before the records existed: tools/make_engine_state_golden.py ran
them on that build and wrote tests/golden/engine_call_sequences.json (codes and error texts only; one answer was rewritten when the
plain and the deep text backward became one entry, see text_deep_forward_needs_the_deep_backward).  BY_DESIGN sequences are those where
that build was unsound (it ran a backward over buffers no forward had written) or whose calls its entries could not express (text jobs
since MvlptTextJob), so their expectation is written down here, with the reason.

Steps that are tuples check buffers between calls: ("keep", buffer, tag) remembers a copy, ("same", buffer, tag) compares with it bit
for bit, ("fill_nan", buffer) / ("all_nan", buffer) bracket a call that must not launch, ("fresh", buffer) compares with the same
buffer of an engine that has seen nothing but one good saved image forward and its backward."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_call_sequences.json")
B, NC, L, N_CTX, N_VPT, N_DEEP = 2, 3, 8, 2, 3, 2
VOCAB = 64          # a token table of the test's own: the 49 408 rows of CLIP's add nothing here


class Rig:
    """A fresh engine on the architecture of tests/test_hip_act_ckpt.py::_arch(256) (2 image layers of width 128, 5 text layers of
    width 256), every buffer the calls need, and the calls by name.  Each call returns the C entry's return code."""

    _sd = None

    def __init__(self):
        from mvlpt_amd import _lib
        from mvlpt_amd.engine import Engine, _ptr, _stream
        from mvlpt_amd.model import build_prompt_layout
        from mvlpt_amd.weights import make_state_dict
        from tests.test_hip_act_ckpt import _arch
        arch = _arch(256)
        if Rig._sd is None:
            Rig._sd = {k: v.to(DEV) for k, v in make_state_dict(arch, 21).items()}
        g = torch.Generator().manual_seed(31)
        rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(DEV)
        self.eng = eng = Engine.from_state_dict(Rig._sd, "fp16", DEV, arch=arch)
        eng.load_token_embedding(rnd(VOCAB, 256, scale=0.02))
        self.h = h = eng.h
        lib, dv, dt, e = _lib.lib, arch.vision_width, arch.transformer_width, arch.embed_dim
        # image side
        image = rnd(B, 3, arch.image_resolution, arch.image_resolution).half()
        vpt, bad_masks = rnd(N_VPT, dv, scale=0.1), torch.ones(2, B + 1, N_VPT, dv, device=DEV)
        feat_i, dfeat_i, dvpt = torch.zeros(B, e, device=DEV), rnd(B, e), torch.zeros(N_VPT, dv, device=DEV)
        # text side
        name_lens = [1, 2, 1]
        layout = build_prompt_layout(name_lens, N_CTX, L, "end").to(DEV)
        eot = torch.tensor([N_CTX + 2 + k for k in name_lens], dtype=torch.int32, device=DEV)
        prefix, suffix = rnd(NC, 1, dt, scale=0.02), rnd(NC, L - 1 - N_CTX, dt, scale=0.02)
        ctx, ctx_long, ctx_deep = rnd(N_CTX, dt, scale=0.1), rnd(L - 1, dt, scale=0.1), rnd(N_DEEP, N_CTX, dt, scale=0.1)
        ctx_csc, ctx_grp = rnd(NC, N_CTX, dt, scale=0.1), rnd(B, N_CTX, dt, scale=0.1)
        feat_t, dfeat_t = torch.zeros(NC, e, device=DEV), rnd(NC, e)
        dctx, dctx_deep = torch.zeros(N_CTX, dt, device=DEV), torch.zeros(N_DEEP, N_CTX, dt, device=DEV)
        ids = torch.randint(1, VOCAB - 1, (NC, L), generator=g, dtype=torch.int32)
        ids[torch.arange(NC), torch.tensor([4, 6, 5])] = VOCAB - 1          # the EOT token: the row maximum
        ids = ids.contiguous()
        # head
        img_f, txt_f, txt_r = rnd(B, e), rnd(NC, e), rnd(4, e)
        logits, dlogits = torch.zeros(B, NC, device=DEV), rnd(B, NC)
        dimg, dtxt, dtxt_r = torch.zeros(B, e, device=DEV), torch.zeros(NC, e, device=DEV), torch.zeros(4, e, device=DEV)
        lo, hi, hi_bad = (C.c_int32 * B)(0, 1), (C.c_int32 * B)(2, 3), (C.c_int32 * B)(2, NC + 1)      # 2 + 2 = 4 text rows
        self.buffers = {"feat_i": feat_i, "dvpt": dvpt, "feat_t": feat_t, "dctx": dctx, "dctx_deep": dctx_deep}
        self._alive = (image, vpt, bad_masks, dfeat_i, layout, eot, prefix, suffix, ctx, ctx_long, ctx_deep, ctx_csc, ctx_grp, dfeat_t, ids, img_f, txt_f,
                       txt_r, logits, dlogits, dimg, dtxt, dtxt_r, lo, hi, hi_bad)
        half = _lib.DT_F16

        def image_fwd(save, prompts=True):
            return lambda: lib.mvlpt_image_fwd(h, _ptr(image), half, _ptr(vpt) if prompts else None, None, N_VPT if prompts else 0, 0, B,
                                               _ptr(feat_i), save, _stream())

        def text_fwd(save, c=ctx, n=N_CTX, **fields):
            job = _lib.MvlptTextJob(prefix=prefix.data_ptr(), suffix=suffix.data_ptr(), ctx=c.data_ptr(), n_ctx=n, layout=layout.data_ptr(),
                                    eot=eot.data_ptr(), n_cls=NC, L=L, save_for_bwd=save, **fields)
            return lambda: lib.mvlpt_text_fwd(h, C.byref(job), _ptr(feat_t), _stream())

        deep = dict(ctx_deep=ctx_deep.data_ptr(), n_deep=N_DEEP)

        self.calls = {
            "set_activation": lambda: lib.mvlpt_set_activation(h, _lib.ACT_QUICKGELU),
            "act_ckpt_1": lambda: lib.mvlpt_set_text_act_ckpt(h, 1),
            "act_ckpt_3": lambda: lib.mvlpt_set_text_act_ckpt(h, 3),
            # image
            "image_fwd": image_fwd(0, prompts=False),
            "image_fwd_save": image_fwd(1),
            "image_fwd_begin": lambda: lib.mvlpt_image_fwd_begin(h, _ptr(image), half, None, None, 0, 0, B, 0, 1, _stream()),
            "image_fwd_resume": lambda: lib.mvlpt_image_fwd_resume(h, _ptr(feat_i), _stream()),
            "image_fwd_abandon": lambda: lib.mvlpt_image_fwd_abandon(h),
            "image_bwd": lambda: lib.mvlpt_image_bwd(h, _ptr(dfeat_i), _ptr(dvpt), None, _stream()),
            "set_vpt_dropout_other_batch": lambda: lib.mvlpt_set_vpt_dropout(h, _ptr(bad_masks), *bad_masks.shape),
            # text
            "text_fwd": text_fwd(0),
            "text_fwd_save": text_fwd(1),
            "text_fwd_save_n_ctx_too_long": text_fwd(1, ctx_long, L - 1),
            "text_fwd_deep_save": text_fwd(1, **deep),
            # jobs no earlier entry could express
            "text_fwd_deep_ranged": text_fwd(1, ctx_grp, class_lo=lo, class_hi=hi, groups=B, **deep),
            "text_fwd_deep_per_class": text_fwd(1, ctx_csc, ctx_per_class=1, **deep),
            "text_fwd_lo_without_hi": text_fwd(1, ctx_grp, class_lo=lo, groups=B),
            "text_encode_tokens": lambda: lib.mvlpt_text_encode_tokens(h, C.c_void_p(ids.data_ptr()), L, NC, L, _ptr(feat_t), _stream()),
            "text_bwd": lambda: lib.mvlpt_text_bwd(h, _ptr(dfeat_t), _ptr(dctx), None, _stream()),
            "text_bwd_deep": lambda: lib.mvlpt_text_bwd(h, _ptr(dfeat_t), _ptr(dctx), _ptr(dctx_deep), _stream()),
            # head
            "logits_fwd": lambda: lib.mvlpt_logits_fwd(h, _ptr(img_f), _ptr(txt_f), 10.0, None, None, B, NC, _ptr(logits), _stream()),
            "logits_bwd": lambda: lib.mvlpt_logits_bwd(h, _ptr(dlogits), _ptr(dimg), _ptr(dtxt), _stream()),
            "logits_ranged_fwd": lambda: lib.mvlpt_logits_ranged_fwd(h, _ptr(img_f), _ptr(txt_r), 10.0, lo, hi, B, NC, _ptr(logits), _stream()),
            "logits_ranged_fwd_bad_range": lambda: lib.mvlpt_logits_ranged_fwd(h, _ptr(img_f), _ptr(txt_r), 10.0, lo, hi_bad, B, NC,
                                                                             _ptr(logits), _stream()),
            "logits_ranged_bwd": lambda: lib.mvlpt_logits_ranged_bwd(h, _ptr(dlogits), _ptr(dtxt_r), _ptr(dimg), _stream()),
        }


class ResNetRig:
    """The engine of tests/test_hip_resnet.py::tiny: a frozen, forward-only image tower."""

    def __init__(self):
        from mvlpt_amd import _lib
        from mvlpt_amd.engine import Engine, _ptr, _stream
        from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
        arch = RESNET_ARCHS["tiny-rn"]
        self.eng = Engine.from_state_dict(make_state_dict(arch, 1), "fp16", DEV, arch=arch)
        self.h = h = self.eng.h
        image = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV)
        feat, dfeat = torch.zeros(B, arch.embed_dim, device=DEV), torch.ones(B, arch.embed_dim, device=DEV)
        self.buffers, self._alive = {"feat_i": feat}, (image, dfeat)
        self.calls = {
            "image_fwd": lambda: _lib.lib.mvlpt_image_fwd(h, _ptr(image), _lib.DT_F32, None, None, 0, 0, B, _ptr(feat), 0, _stream()),
            "image_bwd": lambda: _lib.lib.mvlpt_image_bwd(h, _ptr(dfeat), None, None, _stream()),
        }


# name -> (rig, steps).  Every sequence starts on a fresh engine.
RECORDED = {
    "backward_without_forward": (Rig, ["image_bwd", "text_bwd", "text_bwd_deep", "logits_bwd", "logits_ranged_bwd"]),
    "backward_after_a_forward_that_saved_nothing": (Rig, ["image_fwd", "image_bwd", "text_fwd", "text_bwd", "text_bwd_deep"]),
    "text_backward_twice_act_ckpt_1": (Rig, ["act_ckpt_1", "text_fwd_save", "text_bwd", ("keep", "dctx", "first"), "text_bwd",
                                             ("same", "dctx", "first")]),
    "text_backward_twice_act_ckpt_3": (Rig, ["act_ckpt_3", "text_fwd_save", "text_bwd", ("fill_nan", "dctx"), "text_bwd", ("all_nan", "dctx")]),
    "text_deep_forward_needs_the_deep_backward": (Rig, ["text_fwd_deep_save", "text_bwd", "text_bwd_deep"]),
    "text_forward_refused_for_its_arguments_keeps_the_saved_one": (
        Rig, ["text_fwd_save", "text_bwd", ("keep", "dctx", "before"), "text_fwd_save_n_ctx_too_long", "text_bwd", ("same", "dctx", "before")]),
    "text_encode_tokens_replaces_the_saved_forward": (Rig, ["text_fwd_save", "text_encode_tokens", "text_bwd"]),
    "head_backward_of_the_other_kind": (Rig, ["logits_fwd", "logits_ranged_bwd", "logits_bwd", "logits_bwd", "logits_ranged_fwd", "logits_bwd",
                                              "logits_ranged_bwd"]),
    "head_forward_refused_for_its_ranges": (Rig, ["logits_fwd", "logits_ranged_fwd_bad_range", "logits_bwd"]),
    "set_activation_in_every_image_phase": (
        Rig, ["set_activation", "image_fwd_begin", "set_activation", "image_fwd_abandon", "set_activation", "image_fwd_begin",
              "image_fwd_resume", "set_activation", "image_fwd_save", "set_activation", "image_bwd", "set_activation", "image_bwd"]),
    "set_activation_in_every_text_phase": (
        Rig, ["set_activation", "text_fwd", "set_activation", "text_fwd_save", "set_activation", "text_bwd", "set_activation", "act_ckpt_3",
              "text_fwd_save", "set_activation", "text_bwd", "set_activation", "text_bwd", "act_ckpt_1"]),
    "image_pending_forward": (Rig, ["image_fwd_begin", "image_bwd", "image_fwd_begin", "image_fwd", "image_fwd_abandon", "image_fwd_resume"]),
    "resnet_forward_then_backward": (ResNetRig, ["image_fwd", "image_bwd"]),
}

ERR_ARG, ERR_STATE = -1, -3          # MVLPT_ERR_*
_REFUSED_FWD = ["set_vpt_dropout_other_batch", "image_fwd_save", ("fill_nan", "dvpt"), "image_bwd", ("all_nan", "dvpt")]
_REFUSED_FWD_ANSWERS = [0, (ERR_ARG, "do not match this forward"), (ERR_STATE, "call image_fwd(save_for_bwd=1) first")]
# name -> (reason, steps, expected answer per call: 0, or (code, substring of the error))
BY_DESIGN = {
    "A_forward_refused_behind_the_carve": (
        "the mask check sits behind the workspace carve; the earlier library had marked the record saved at the carve and ran this "
        "backward over a workspace no forward had written",
        _REFUSED_FWD, _REFUSED_FWD_ANSWERS),
    "B_forward_refused_behind_the_carve_after_a_saved_one": (
        "the refused forward's carve has overwritten the activations of the saved forward in front of it, so that one is gone too; the "
        "engine is as good as new afterwards",
        ["image_fwd_save"] + _REFUSED_FWD + ["image_fwd_save", ("fresh", "feat_i"), "image_bwd", ("fresh", "dvpt")],
        [0] + _REFUSED_FWD_ANSWERS + [0, 0]),
    "C_text_jobs_no_earlier_entry_could_express": (
        "refused for their fields before any engine state is touched: the saved forward in front of them keeps its backward, bit for bit",
        ["text_fwd_save", "text_bwd", ("keep", "dctx", "saved"),
         "text_fwd_deep_ranged", "text_bwd", ("same", "dctx", "saved"),
         "text_fwd_deep_per_class", "text_bwd", ("same", "dctx", "saved"),
         "text_fwd_lo_without_hi", "text_bwd", ("same", "dctx", "saved")],
        [0, 0, (ERR_ARG, "not offered on the ranged tower"), 0, (ERR_ARG, "generic context"), 0, (ERR_ARG, "come together"), 0]),
    "D_text_bwd_without_dctx_deep_after_a_deep_forward": (
        "dctx_deep is required exactly when the saved forward ran deep prompts; the refusal launches nothing and the right call that "
        "follows gives the gradients of a run without the refused call",
        ["text_fwd_deep_save", "text_bwd_deep", ("keep", "dctx", "clean"), ("keep", "dctx_deep", "clean_deep"),
         "text_fwd_deep_save", ("fill_nan", "dctx"), "text_bwd", ("all_nan", "dctx"),
         "text_bwd_deep", ("same", "dctx", "clean"), ("same", "dctx_deep", "clean_deep")],
        [0, 0, 0, (ERR_ARG, "dctx_deep is null after a forward with deep prompts"), 0]),
    "E_text_bwd_with_dctx_deep_after_a_forward_without_deep_prompts": (
        "dctx_deep must be null when the saved forward ran no deep prompts; as above",
        ["text_fwd_save", "text_bwd", ("keep", "dctx", "clean"),
         "text_fwd_save", ("fill_nan", "dctx"), ("fill_nan", "dctx_deep"), "text_bwd_deep", ("all_nan", "dctx"), ("all_nan", "dctx_deep"),
         "text_bwd", ("same", "dctx", "clean")],
        [0, 0, 0, (ERR_ARG, "dctx_deep is set after a forward without deep prompts"), 0]),
}


def run_sequence(rig, steps, fresh=None):
    """-> [[call, return code, error text of a refusal or ""]] of the calls; the buffer checks in between are asserted here."""
    from mvlpt_amd import _lib
    answers, kept = [], {}
    for step in steps:
        if isinstance(step, str):
            rc = rig.calls[step]()
            answers.append([step, rc, _lib.last_error(rig.h) if rc else ""])
            continue
        torch.cuda.synchronize()
        what, buf = step[0], rig.buffers[step[1]]
        if what == "keep":
            kept[step[2]] = buf.clone()
        elif what == "same":
            assert bool(torch.isfinite(buf).all()) and torch.equal(buf, kept[step[2]]), f"{step[1]} differs from the one kept as {step[2]!r}"
        elif what == "fill_nan":
            buf.fill_(float("nan"))
        elif what == "all_nan":
            assert bool(torch.isnan(buf).all()), f"{step[1]}: a refused call has written its output"
        elif what == "fresh":
            assert bool(torch.isfinite(buf).all()) and torch.equal(buf, fresh.buffers[step[1]]), f"{step[1]} differs from a fresh engine's"
        else:
            raise ValueError(step)
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    return answers


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_the_recorded_sequences(golden):
    assert set(golden) == set(RECORDED)
    for name, (_, steps) in RECORDED.items():
        assert [a[0] for a in golden[name]] == [s for s in steps if isinstance(s, str)], name
    assert not set(BY_DESIGN) & set(golden), "a sequence the earlier library was unsound on must not be recorded from it"


@pytest.mark.parametrize("name", list(RECORDED))
def test_recorded_sequence_answers_as_before(golden, name):
    make_rig, steps = RECORDED[name]
    got = run_sequence(make_rig(), steps)
    assert len(got) == len(golden[name])
    for i, ((call, rc, err), (_, want_rc, want_err)) in enumerate(zip(got, golden[name])):
        print(f"{name}[{i}] {call}: {rc} {err!r}")
        assert rc == want_rc and want_err in err, f"{name}: call {i} ({call}) answered {rc} {err!r}, recorded {want_rc} {want_err!r}"


@pytest.fixture(scope="module")
def fresh():
    rig = Rig()
    assert [a[1] for a in run_sequence(rig, ["image_fwd_save", "image_bwd"])] == [0, 0]
    return rig


@pytest.mark.parametrize("name", list(BY_DESIGN))
def test_sequence_expected_by_design(fresh, name):
    reason, steps, want = BY_DESIGN[name]
    got = run_sequence(Rig(), steps, fresh)
    assert len(got) == len(want)
    for i, ((call, rc, err), w) in enumerate(zip(got, want)):
        want_rc, want_err = w if isinstance(w, tuple) else (w, "")
        print(f"{name}[{i}] {call}: {rc} {err!r}")
        assert rc == want_rc and want_err in err, f"{name}: call {i} ({call}) answered {rc} {err!r}, expected {want_rc} {want_err!r} ({reason})"
