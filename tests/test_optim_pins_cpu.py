"""Pins for the capturable forms of optim.Adam, on the CPU (the recorder fixture and the 384-float arena of
test_optim_segments_cpu.py): the full call log of a full and a partial step with the tensors every lr_schedule launch
receives, the structure of state_dict()['gdn'] after those two steps, and a checkpoint written out by hand in the layout of
revision 1 of that key that must load, continue with the recorded calls and come back byte for byte.  The expected values
are literals recorded at the commit before the device tables of plain and segmented stores became one type."""
import struct

import pytest
import torch

from test_optim_segments_cpu import GUARD_EMA, HYPER, _arena_and_net, _two_groups, calls      # noqa: F401  (calls: a fixture)

SCHED = {"kind": "cosine", "warmup": 3, "total": 8, "floor": 0.1}
FORMS = {
    "capturable": (False, dict(capturable=True)),
    "guard_ema": (False, dict(GUARD_EMA)),
    "schedule": (False, dict(schedule=SCHED)),
    "segmented": (True, dict(segmented=True)),
    "seg_sched": (True, dict(segmented=True, schedule=SCHED)),
    "seg_sched_guard_ema": (True, dict(segmented=True, schedule=SCHED, **GUARD_EMA)),
}
STEP_FMT = "<ddiff"


@pytest.fixture
def log(calls, monkeypatch):      # noqa: F811
    from gdn_amd import ops
    monkeypatch.setattr(ops, "lr_schedule", lambda hyper, base, states, kind, warmup, total, floor: calls.append(
        ("lr_schedule", hyper, base, states, (kind, warmup, total, floor))))
    return calls


def _make(form):
    from gdn_amd.optim import Adam
    two, kw = FORMS[form]
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net, freeze=False) if two else net.parameters(), **HYPER, **kw)
    return net, ar, opt


def _described(log, opt, ar, net):
    """The log with the tensors of every lr_schedule call named: (numel, float offset into the store's hyper table),
    (numel, double offset into its base rates) and the step states -- ('states', numel, byte offset into the table of a
    plan), ('state', numel) for a plain store's own, ('pdev', k) for the own state of parameters()[k]."""
    st = opt.store_of(ar)
    ps = list(net.parameters())
    hyper = st.plan.hyper if st.plan is not None else st.hyper
    base = st.plan.base_lr if st.plan is not None else st.base_lr
    out = []
    for c in log:
        if c[0] != "lr_schedule":
            out.append(c)
            continue
        _, h, b, s, sched = c
        who = None
        if st.plan is not None and st.plan.states is not None and \
                0 <= s.data_ptr() - st.plan.states.data_ptr() < st.plan.states.numel():
            who = ("states", s.numel(), s.data_ptr() - st.plan.states.data_ptr())
        elif st.plan is None and st.state is not None and s.data_ptr() == st.state.data_ptr():
            who = ("state", s.numel())
        else:
            (k,) = [k for k, p in enumerate(ps) if id(p) in st.pdev and st.pdev[id(p)] is s]
            who = ("pdev", k)
        assert h.dtype == torch.float32 and b.dtype == torch.float64 and s.dtype == torch.uint8
        out.append(("lr_schedule", (h.numel(), (h.data_ptr() - hyper.data_ptr()) // 4),
                    (b.numel(), (b.data_ptr() - base.data_ptr()) // 8), who, sched))
    return out


def _shape(x):
    """A structure with every tensor replaced by (dtype, numel)."""
    if isinstance(x, torch.Tensor):
        return (str(x.dtype), x.numel())
    if isinstance(x, dict):
        return {k: _shape(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_shape(v) for v in x]
    return x


def _counts(sd):
    """Every count a state_dict() carries: 'step' of each entry, and the t of every device step state of the records."""
    t = lambda b, o=0: struct.unpack_from(STEP_FMT, bytes(b.tolist()), o)[2]      # noqa: E731
    out = {"state": {k: float(s["step"]) for k, s in sd["state"].items()}, "stores": []}
    for rec in sd["gdn"]["stores"]:
        seg = rec.get("seg")
        out["stores"].append({"state": None if rec["state"] is None else t(rec["state"]),
                              "pdev": {k: t(b) for k, b in rec["pdev"].items()},
                              "seg": None if seg is None or seg["states"] is None else
                              [t(seg["states"], 32 * g) for g in range(seg["states"].numel() // 32)]})
    return out


def _two_steps(form, log):
    net, ar, opt = _make(form)
    opt.step()
    list(net.parameters())[2].grad = None
    opt.step()
    return net, ar, opt


# ---- 1. the call log, and what every lr_schedule launch receives ---------------------------------------------------------
MAP2 = [0, 0, 1, 1, 0, 0]
CS = ("cosine", 3, 8, 0.1)
COVERED = [(0, 54, 0, 0), (64, 3, 0, 1), (192, 3, 1, 3), (256, 54, 0, 4), (320, 2, 0, 5)]      # offset, numel, table row, parameters() index
LOGS = {
    "capturable": [("adam_step_dev", 384, 0)] + [("adam_step_dev", n, o) for o, n, _, _ in COVERED],
    "guard_ema": [("grad_sumsq", 384, False), ("grad_guard_finalize",), ("adam_step_dev_guarded", 384, 0), ("ema_update", 384, 0)]
    + [("grad_sumsq", n, i > 0) for i, (o, n, _, _) in enumerate(COVERED)] + [("grad_guard_finalize",)]
    + [c for o, n, _, _ in COVERED for c in (("adam_step_dev_guarded", n, o), ("ema_update", n, o))],
    "schedule": [("lr_schedule", (6, 0), (1, 0), ("state", 28), CS), ("adam_step_dev", 384, 0)]
    + [c for o, n, _, k in COVERED for c in (("lr_schedule", (6, 0), (1, 0), ("pdev", k), CS), ("adam_step_dev", n, o))],
    "segmented": [("adam_step_seg", 384, MAP2, (2, 6), 64, False)] + [("adam_step_dev", n, o) for o, n, _, _ in COVERED],
    "seg_sched": [("lr_schedule", (12, 0), (2, 0), ("states", 64, 0), CS), ("adam_step_seg", 384, MAP2, (2, 6), 64, False)]
    + [c for o, n, r, k in COVERED for c in (("lr_schedule", (6, 6 * r), (1, r), ("pdev", k), CS), ("adam_step_dev", n, o))],
    "seg_sched_guard_ema": [("grad_sumsq_seg", 384, MAP2, False), ("grad_guard_finalize",),
                            ("lr_schedule", (12, 0), (2, 0), ("states", 64, 0), CS),
                            ("adam_step_seg", 384, MAP2, (2, 6), 64, True), ("ema_update_seg", 384, MAP2, 64, True)]
    + [("grad_sumsq", n, i > 0) for i, (o, n, _, _) in enumerate(COVERED)] + [("grad_guard_finalize",)]
    + [c for o, n, r, k in COVERED for c in (("lr_schedule", (6, 6 * r), (1, r), ("pdev", k), CS),
                                             ("adam_step_dev_guarded", n, o), ("ema_update", n, o))],
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_full_then_partial_step_call_log(log, form):
    net, ar, opt = _two_steps(form, log)
    assert _described(log, opt, ar, net) == LOGS[form]


# ---- 2. the checkpoint's shape -------------------------------------------------------------------------------------------
U8 = ("torch.uint8", 28)
PLAIN_REC = {"kind": "arena", "params": [0, 1, 2, 3, 4, 5], "step": 1, "pstep": [2, 2, 1, 2, 2, 2], "full_dev": True, "state": U8,
             "pdev": {0: U8, 1: U8, 3: U8, 4: U8, 5: U8}}
# (a segmented optimizer's parameters are numbered in group order: conv weights and biases 0-3, gamma 4, beta 5)
SEG_REC = {"kind": "arena", "params": [0, 1, 4, 5, 2, 3], "step": 2, "pstep": [2, 2, 1, 2, 2, 2], "full_dev": True, "state": None,
           "pdev": {0: U8, 1: U8, 5: U8, 2: U8, 3: U8}, "seg": {"key": [0, 0, 1, 1, 0, 0], "states": ("torch.uint8", 64)}}
GUARD = {"max_grad_norm": 1.0, "skip_nonfinite": True, "steps": 0, "clipped": 0, "skipped": 0}
EMA = {"decay": 0.99, "avg": {0: ("torch.float32", 54), 1: ("torch.float32", 3), 2: ("torch.float32", 3), 3: ("torch.float32", 3),
                              4: ("torch.float32", 54), 5: ("torch.float32", 2)}}
EMA_SEG = {"decay": 0.99, "avg": {0: ("torch.float32", 54), 1: ("torch.float32", 3), 2: ("torch.float32", 54), 3: ("torch.float32", 2),
                                  4: ("torch.float32", 3), 5: ("torch.float32", 3)}}
HEAD = {"version": 1, "capturable": True, "grad_scale": 1.0}
SHAPES = {
    "capturable": dict(HEAD, stores=[PLAIN_REC]),
    "guard_ema": dict(HEAD, stores=[PLAIN_REC], guard=GUARD, ema=EMA),
    "schedule": dict(HEAD, stores=[PLAIN_REC], schedule=SCHED),
    "segmented": dict(HEAD, stores=[SEG_REC]),
    "seg_sched": dict(HEAD, stores=[SEG_REC], schedule=SCHED),
    "seg_sched_guard_ema": dict(HEAD, stores=[SEG_REC], guard=GUARD, schedule=SCHED, ema=EMA_SEG),
}
# the recorders launch nothing, so a device count stays what the host wrote there: 0 in the store's own state (made before the
# first update), 1 in each parameter's (cloned from it, or made for pstep - 1); the adam_step_seg recorder counts as the kernel does
PLAIN_COUNTS = {"state": {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0, 5: 0.0},
                "stores": [{"state": 0, "pdev": {0: 0, 1: 0, 3: 0, 4: 0, 5: 0}, "seg": None}]}
SEG_COUNTS = {"state": {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0, 5: 1.0},
              "stores": [{"state": None, "pdev": {0: 1, 1: 1, 5: 1, 2: 1, 3: 1}, "seg": [1, 1]}]}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_checkpoint_shape_after_a_full_and_a_partial_step(log, form):
    net, ar, opt = _two_steps(form, log)
    sd = opt.state_dict()
    assert _shape(sd["gdn"]) == SHAPES[form]
    assert list(sd["gdn"]) == list(SHAPES[form]) and [list(r) for r in sd["gdn"]["stores"]] == [list(r) for r in SHAPES[form]["stores"]]
    assert _counts(sd) == (SEG_COUNTS if FORMS[form][0] else PLAIN_COUNTS)
    st = opt.store_of(ar)
    assert [st.count(p) for p in net.parameters()] == ([1] * 6 if FORMS[form][0] else [0] * 6)
    assert (st.pstep is not None) and [st.pstep[id(p)] for p in net.parameters()] == [2, 2, 1, 2, 2, 2]


# ---- 3. a checkpoint of the parent revision, written out by hand ---------------------------------------------------------
def _state28(t, b1=0.9, b2=0.999, host=False):
    """A step state after t updates as the device leaves it, or (host) as the host makes one: no bias corrections yet."""
    p1, p2 = b1 ** t, b2 ** t
    bc = (0.0, 0.0) if host else (1.0 - p1, (1.0 - p2) ** 0.5)
    return torch.frombuffer(bytearray(struct.pack(STEP_FMT, p1, p2, t, *bc)), dtype=torch.uint8)


def _checkpoint(form):
    """What the parent revision's state_dict() holds after three full steps and one without a gradient for parameters()[2]
    (device counts 3 in the store's or the groups' states, 4 in the parameters' own), tensors small and recognisable."""
    two, kw = FORMS[form]
    shapes = [(3, 2, 3, 3), (3,), (3,), (3,), (3, 2, 3, 3), (2,)]              # parameters() order
    order = [0, 1, 4, 5, 2, 3] if two else [0, 1, 2, 3, 4, 5]                   # saved index -> parameters() index
    steps = [4, 4, 3, 4, 4, 4]                                                  # parameters() order
    state = {i: {"step": torch.tensor(float(steps[k])), "exp_avg": torch.full(shapes[k], 0.01 * (k + 1)),
                 "exp_avg_sq": torch.full(shapes[k], 0.001 * (k + 1))} for i, k in enumerate(order)}
    saved = {k: i for i, k in enumerate(order)}                                 # parameters() index -> saved index
    rec = {"kind": "arena", "params": [saved[k] for k in range(6)], "step": 4 if two else 3, "pstep": list(steps), "full_dev": True,
           "state": None if two else _state28(3), "pdev": {saved[k]: _state28(4) for k in (0, 1, 3, 4, 5)}}
    if two:
        rec["seg"] = {"key": [0, 0, 1, 1, 0, 0], "states": torch.cat([_state28(3), torch.zeros(4, dtype=torch.uint8)] * 2)}
    groups = [dict(HYPER, betas=(0.8999999761581421, 0.9990000128746033), params=[0, 1, 2, 3, 4, 5])]
    if two:
        groups = [dict(groups[0], params=[0, 1, 2, 3]), dict(groups[0], params=[4, 5], lr_mult=0.5, weight_decay=0.0)]
    gdn = {"version": 1, "capturable": True, "grad_scale": 0.5, "stores": [rec]}
    if "max_grad_norm" in kw:
        gdn["guard"] = {"max_grad_norm": 1.0, "skip_nonfinite": True, "steps": 5, "clipped": 2, "skipped": 1}
    if "schedule" in kw:
        gdn["schedule"] = dict(SCHED)
    if "ema_decay" in kw:
        gdn["ema"] = {"decay": 0.99, "avg": {i: torch.full(shapes[k], 0.5 + k) for i, k in enumerate(order)}}
    return {"state": state, "param_groups": groups, "gdn": gdn}


def _same(a, b, path="gdn"):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, k))
    else:
        assert a == b, path


# the step after the load, every parameter with a gradient: per tensor, since per-parameter device states exist
ALL = [(0, 54, 0, 0), (64, 3, 0, 1), (128, 3, 1, 2), (192, 3, 1, 3), (256, 54, 0, 4), (320, 2, 0, 5)]
NEXT = {
    "capturable": [("adam_step_dev", n, o) for o, n, _, _ in ALL],
    "guard_ema": [("grad_sumsq", n, i > 0) for i, (o, n, _, _) in enumerate(ALL)] + [("grad_guard_finalize",)]
    + [c for o, n, _, _ in ALL for c in (("adam_step_dev_guarded", n, o), ("ema_update", n, o))],
    "schedule": [c for o, n, _, k in ALL for c in (("lr_schedule", (6, 0), (1, 0), ("pdev", k), CS), ("adam_step_dev", n, o))],
    "segmented": [("adam_step_dev", n, o) for o, n, _, _ in ALL],
    "seg_sched": [c for o, n, r, k in ALL for c in (("lr_schedule", (6, 6 * r), (1, r), ("pdev", k), CS), ("adam_step_dev", n, o))],
    "seg_sched_guard_ema": [("grad_sumsq", n, i > 0) for i, (o, n, _, _) in enumerate(ALL)] + [("grad_guard_finalize",)]
    + [c for o, n, r, k in ALL for c in (("lr_schedule", (6, 6 * r), (1, r), ("pdev", k), CS),
                                         ("adam_step_dev_guarded", n, o), ("ema_update", n, o))],
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_parent_checkpoint_loads_continues_and_comes_back(log, form):
    two = FORMS[form][0]
    ckpt = _checkpoint(form)
    net, ar, opt = _make(form)
    opt.load_state_dict(ckpt)
    # before any step: handed back as it was read
    sd = opt.state_dict()
    _same(sd["gdn"], ckpt["gdn"])
    _same(sd["state"], ckpt["state"], "state")
    # the next step: the recorded calls, on stores that took the record's bytes
    opt.step()
    assert _described(log, opt, ar, net) == NEXT[form]
    st = opt.store_of(ar)
    ps = list(net.parameters())
    # plain: the device's own counts (the recorders launch nothing); a plan without group states counts on the host
    assert [st.count(p) for p in ps] == ([5, 5, 4, 5, 5, 5] if two else [4, 4, 3, 4, 4, 4])
    assert [st.pstep[id(p)] for p in ps] == [5, 5, 4, 5, 5, 5]
    # ... and come back: the same bytes, one more per-parameter state (parameters()[2]'s: a copy of the plain store's own
    # state, which one-launch updates drove; made on the host for 3 updates where a plan has no group states, as one built
    # beside per-parameter states has none) and the host counts of one more update
    back = opt.state_dict()
    want = _checkpoint(form)
    rec = want["gdn"]["stores"][0]
    rec["pstep"] = [5, 5, 4, 5, 5, 5]
    k2 = rec["params"][2]                                           # parameters()[2]'s number in the param groups
    rec["pdev"] = {k: (rec["pdev"][k] if k != k2 else _state28(3, host=two)) for k in rec["params"]}
    if two:
        rec["step"] = 5
        rec["seg"]["states"] = None
    # (the guard's counts wait for the first guarded update's record; the averages went through the store's buffer and back)
    _same(back["gdn"], want["gdn"])
    assert {k: float(s["step"]) for k, s in back["state"].items()} == {k: float(s["step"]) + two for k, s in ckpt["state"].items()}
    for k in ckpt["state"]:
        assert torch.equal(back["state"][k]["exp_avg"], ckpt["state"][k]["exp_avg"])
        assert torch.equal(back["state"][k]["exp_avg_sq"], ckpt["state"][k]["exp_avg_sq"])
