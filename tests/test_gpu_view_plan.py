"""The walk plan of a cached view (include/lsr.h: lsr_view_plan_pack_bytes, lsr_view_bind): the
instances' cover masks, which a compositing derives from the frozen geometry alone, are saved with the
view's pack, and a set bound to such a pack composites and replays from them: the render forward
neither computes nor stores them, the backward reads them from the pack.  Everything else a compositing
leaves for the backward (final_T, n_contrib, split descriptors, the class lists and counts) is rebuilt
in the set at every step, as on a miss.  A hit must give what a miss gives.

Shapes: tests/test_gpu_view_cache.py's 70 x 50 with 1501 Gaussians and 17 x 33 with 302 (neither side
a multiple of 16: threads outside the image in the edge tiles), and a 48 x 32 scene of 3000
low-opacity Gaussians around the image centre, whose tiles hold more than 512 list entries and whose
pixels composite past the 256-, 512- and 768-entry boundaries (split replay; asserted below from the
forward's own ranges and n_contrib).

Exact outputs are compared bit for bit; gradients -- sums of float atomics -- with assert_grad_close,
the project's 1e-4 bar.
"""
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.render import render
from tests.scenes import scene
from tests.test_gpu_captured_forms import _adam, _frozen_model, _state, assert_states_close
from tests.test_gpu_fused import _Opt, _Pipe
from tests.test_gpu_parity import assert_grad_close
from tests.test_gpu_view_bind import _backward_only, _bind, _blank_bound, _bound_set, _run
from tests.test_gpu_view_cache import COMPOSITE, DEV, SEQ, _Case, _gaussians, _views
from langsplat_amd.pipeline import PipelinedGraphStep

pytestmark = pytest.mark.gpu
GEOM, IMAGE, BINNING = _native.LSR_BUF_GEOM, _native.LSR_BUF_IMAGE, _native.LSR_BUF_BINNING
PLAN_ON = 1  # the table's plan word (include/lsr.h)


def _split_scene():
    st, inp = scene(P=3000, W=48, H=32, seed=7, extent=0.6, scale_range=(0.1, 0.3))
    inp["opacities"] = torch.full_like(inp["opacities"], 0.03)
    return st, inp


def _scene_of(name):
    if name == "70x50":
        return scene(P=1501, W=70, H=50, seed=4, scale_range=(0.03, 0.2))
    if name == "17x33":
        return scene(P=302, W=17, H=33, seed=4, scale_range=(0.03, 0.2))
    return _split_scene()


SHAPES = ["70x50", "17x33", "split"]


class _Plan:
    """Views of the plan's arrays: in a buffer set (the ones a miss writes) and in a pack."""

    def __init__(self, case):
        self.case = case
        self.R = case.counts[0]
        self.lay = _native.view_plan_layout(case.P, case.W, case.H, case.cap[0], self.R)
        self.T, self.HW = self.lay["tiles"], case.W * case.H

    def new_pack(self):
        return torch.empty((self.lay["pack_bytes"],), dtype=torch.uint8, device=DEV)

    def _lists(self, counts, words, per_class):
        """The class lists, class by class: `words` is the set's [class][per_class] array."""
        return torch.cat([words[c * per_class:c * per_class + int(n)] for c, n in enumerate(counts.tolist())]
                         + [words[:0]])

    def of_set(self, s):
        L, img, bn = self.lay, s.tensor(IMAGE), s.tensor(BINNING)
        cnt = img[L["set_counters"]:L["set_counters"] + 4 * (16 + 128)].view(torch.int32)
        bwd_counts = cnt[L["word_bwd_class"]:L["word_bwd_class"] + 64].clone()
        per = 4 * self.T
        lists = img[L["set_bwd_lists"]:L["set_bwd_lists"] + 4 * 64 * per].view(torch.int32)
        return {"ready": int(cnt[L["word_plan_ready"]]),
                "cover": bn[L["set_cover"]:L["set_cover"] + self.R].clone(),
                "final_T": img[L["set_final_T"]:L["set_final_T"] + 4 * self.HW].view(torch.int32).clone(),
                "n_contrib": img[L["set_n_contrib"]:L["set_n_contrib"] + 4 * self.HW].view(torch.int32).clone(),
                "split_desc": img[L["set_split_desc"]:L["set_split_desc"] + 16 * self.T].view(torch.int32).clone(),
                "bwd_counts": bwd_counts, "bwd_lists": self._lists(bwd_counts, lists, per)}

    def of_pack(self, pack):
        L = self.lay
        cnt = pack[:4 * 80].view(torch.int32)
        return {"ready": int(cnt[L["word_plan_ready"]]),
                "cover": pack[L["pack_cover"]:L["pack_cover"] + self.R].clone()}

    def loss_code(self, s):
        off = self.lay["set_loss_code"]
        return s.tensor(IMAGE)[off:off + self.HW].clone()

    def ranges(self, s):
        off = self.case.lay["ranges"]
        return s.tensor(IMAGE)[off:off + 8 * self.T].view(torch.int32).view(self.T, 2).cpu()


def _table(case, s):
    """The set's table: (rec01, recb, point_list, s01, sb, cover, plan)."""
    off = _native.view_bind_layout(case.P, case.W, case.H)["table"]
    t = s.tensor(GEOM)[off:off + 48].cpu()
    return (t[:24].view(torch.int64).tolist() + t[24:32].view(torch.int32).tolist()
            + t[32:40].view(torch.int64).tolist() + t[40:44].view(torch.int32).tolist())


def _step(case, plan, s):
    """The composite phase and the language backward on bound set s -> (images and loss, loss codes,
    gradients).  (The backward's state is read by the caller: from the set after a miss, from the
    pack after a hit.)"""
    out = case._forward(s, COMPOSITE)
    nr, color, lang, radii, geom, binning, image = out
    exact = {"color": color.clone(), "language": lang.clone(), "loss": s.loss.clone(), "radii": radii.clone(),
             "loss_code": plan.loss_code(s)}
    return exact, _backward_only(case, out, True)


def _assert_backward_state_equal(plan, mine, got, tag):
    """What a step left in its set for the backward, against the miss's (bit for bit; the lists' order
    within a class is the order of the forward's atomics: compared as sets; a tile's descriptor is
    written only if the tile has work items: item = 4 tile + chunk)."""
    for k in ("final_T", "n_contrib", "bwd_counts"):
        assert torch.equal(got[k], mine[k]), f"{tag}: {k} differs"
    assert torch.equal(got["bwd_lists"].sort().values, mine["bwd_lists"].sort().values), f"{tag}: work items differ"
    desc, first = got["split_desc"].view(plan.T, 4), mine["split_desc"].view(plan.T, 4)
    live = torch.unique(mine["bwd_lists"] // 4).long()
    assert live.numel() > 0 and torch.equal(desc[live, :2], first[live, :2]), f"{tag}: split_desc differs"


def _assert_step_equal(ref, got, tag):
    for k in ref[0]:
        assert torch.equal(ref[0][k], got[0][k]), f"{tag}: {k} differs"
    assert set(ref[1]) == set(got[1])
    for k in ref[1]:
        assert bool(torch.isfinite(got[1][k]).all()), f"{tag}: {k} is not finite"
        assert_grad_close(f"{tag} {k}", got[1][k].cpu().numpy(), ref[1][k].cpu().numpy())


def _miss_then_pack(case, plan):
    """A miss on bound set A (geometry phase, composite, backward) and A's pack with the plan."""
    A = _bound_set()
    case.geometry(A)
    ref = _step(case, plan, A)
    mine = plan.of_set(A)
    assert mine["ready"] == 1, "the render forward did not flag its plan"
    pack = plan.new_pack()
    _native.view_save(_native.view_args(A.bufs, plan.R, pack), torch.cuda.current_stream())
    return A, ref, mine, pack


# ---- 1. a hit equals a miss ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_hit_equals_miss(shape):
    st, inp = _scene_of(shape)
    case = _Case(st, inp, "language")
    plan = _Plan(case)
    A, ref, mine, pack = _miss_then_pack(case, plan)
    assert case.counts[0] > 0 and float(ref[0]["loss"]) > 0
    assert any(float(v.abs().sum()) > 0 for v in ref[1].values())
    # the scene is what the test needs (from the forward's own state)
    n_contrib = mine["n_contrib"].cpu()
    lens = (plan.ranges(A)[:, 1] - plan.ranges(A)[:, 0])
    if shape != "split":
        assert case.W % 16 != 0 and case.H % 16 != 0  # threads outside the image in the edge tiles
    else:
        assert int(lens.max()) > 512, "no tile with more than 512 list entries"
        for bound in (256, 512, 768):
            assert int((n_contrib > bound).sum()) > 0, f"no pixel composites past entry {bound}"
        assert int(((n_contrib > 0) & (n_contrib <= 256)).sum()) > 0  # ... and some end inside the first chunk
        desc = mine["split_desc"].view(plan.T, 4).cpu()
        assert int(desc[lens > 512, 0].max()) == 3, "no tile replays as four chunks"
        assert int(mine["bwd_counts"].sum()) > int((lens > 0).sum()), "no tile has more than one work item"
    # the cover masks the backward of a hit reads are the pack's: bit for bit what the miss wrote into its set
    saved = plan.of_pack(pack)
    assert saved["ready"] == 1
    assert torch.equal(mine["cover"], saved["cover"]), f"{shape}: pack vs the miss's set: cover differs"
    before = pack.clone()

    B = _bound_set()
    case.geometry(B)  # (allocates B at the capacity sizes)
    _blank_bound(case, B, seed=11)  # every byte 0xFF: stale arrays, NaN gradient records
    _bind(case, B, plan.R, pack)
    tab = _table(case, B)
    lo, hi = pack.data_ptr(), pack.data_ptr() + pack.numel()
    assert tab[6] == PLAN_ON, tab
    assert tab[5] - lo == plan.lay["pack_cover"] and lo <= tab[5] < hi, tab
    bound = plan.of_set(B)
    assert bound["ready"] == 0  # (the set's own array holds no plan: a save from it would keep none)
    assert int(bound["bwd_counts"].abs().sum()) == 0  # the compositing adds to them
    got = _step(case, plan, B)
    _assert_step_equal(ref, got, f"{shape}: hit vs miss")
    # read in place: the hit wrote neither the pack nor the set's own cover masks, and did not flag any
    assert torch.equal(pack, before), "the pack was written"
    after = plan.of_set(B)
    assert bool((after["cover"] == 0xFF).all()), "the hit's forward wrote the set's own cover"
    assert after["ready"] == 0
    # the rest of the backward's state: rebuilt in the set, bit for bit the miss's
    _assert_backward_state_equal(plan, mine, after, f"{shape}: hit vs miss")
    # a second hit on the same set (its records hold the first one's sums until the forward clears them)
    _bind(case, B, plan.R, pack)
    _assert_step_equal(ref, _step(case, plan, B), f"{shape}: second hit")
    _assert_backward_state_equal(plan, mine, plan.of_set(B), f"{shape}: second hit")


def test_two_sets_on_one_pack():
    st, inp = _scene_of("70x50")
    case = _Case(st, inp, "language")
    plan = _Plan(case)
    _, ref, _, pack = _miss_then_pack(case, plan)
    before = pack.clone()
    A, B = _bound_set(), _bound_set()
    for s in (A, B):
        case.geometry(s)
        _blank_bound(case, s, seed=12)
        _bind(case, s, plan.R, pack)
    oa = case._forward(A, COMPOSITE)
    ea = {"color": oa[1].clone(), "language": oa[2].clone(), "loss": A.loss.clone(), "radii": oa[3].clone(),
          "loss_code": plan.loss_code(A)}
    got_b = _step(case, plan, B)
    got_a = (ea, _backward_only(case, oa, True))
    _assert_step_equal(ref, got_a, "set A")
    _assert_step_equal(ref, got_b, "set B")
    assert torch.equal(pack, before)


# ---- 2. packs without a plan --------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["saved before any compositing", "no room in the pack"])
def test_pack_without_a_plan_binds_as_before(how):
    st, inp = _scene_of("70x50")
    case = _Case(st, inp, "language")
    plan = _Plan(case)
    A, ref, _, _ = _miss_then_pack(case, plan)
    if how == "no room in the pack":
        pack = torch.empty((_native.view_pack_bytes(case.P, case.W, case.H, plan.R),), dtype=torch.uint8, device=DEV)
    else:
        case.geometry(A)  # again: the geometry phase clears the flag, nothing composited since
        assert plan.of_set(A)["ready"] == 0
        pack = plan.new_pack()
    pack.fill_(0xFF)
    _native.view_save(_native.view_args(A.bufs, plan.R, pack), torch.cuda.current_stream())
    assert int(pack[:64].view(torch.int32)[8]) == 0
    B = _bound_set()
    case.geometry(B)
    _blank_bound(case, B, seed=13)
    _bind(case, B, plan.R, pack)
    tab = _table(case, B)
    assert tab[5:7] == [0, 0], tab
    got = _step(case, plan, B)
    _assert_step_equal(ref, got, how)
    assert plan.of_set(B)["ready"] == 1  # the plain bound form: the forward built the plan in the set


# ---- 3. a miss after a hit ------------------------------------------------------------------------------

def test_miss_after_hit_rebuilds_the_plan():
    """The set a hit ran on gets new geometry (what invalidate_views or an edited tensor leads to): the
    geometry phase's table has no plan, the forward computes, stores and flags everything again, and a
    pack saved from the set then equals the first one."""
    st, inp = _scene_of("split")
    case = _Case(st, inp, "language")
    plan = _Plan(case)
    _, ref, mine, pack = _miss_then_pack(case, plan)
    B = _bound_set()
    case.geometry(B)
    _blank_bound(case, B, seed=14)
    _bind(case, B, plan.R, pack)
    _assert_step_equal(ref, _step(case, plan, B), "hit")
    case.geometry(B)
    tab = _table(case, B)
    assert tab[5:7] == [0, 0] and plan.of_set(B)["ready"] == 0, tab
    _assert_step_equal(ref, _step(case, plan, B), "miss after the hit")
    again = plan.of_set(B)
    assert again["ready"] == 1
    assert torch.equal(again["cover"], mine["cover"])
    _assert_backward_state_equal(plan, mine, again, "miss after the hit")


# ---- 4. the step -------------------------------------------------------------------------------------------

def _plan_words(pg):
    P = int(pg.params[0].shape[0])
    out = []
    for s in pg.sets:
        _, H, W = s.tensors[("out", "color")].shape
        off = _native.view_bind_layout(P, int(W), int(H))["table"]
        out.append(int(s.tensors[("scratch", GEOM)][off + 40:off + 44].view(torch.int32)))
    return out


@pytest.mark.parametrize("what", [None, "invalidate", "edit"])
@pytest.mark.parametrize("wait", [True, False])
def test_step_with_plans_matches_uncached(what, wait, monkeypatch):
    """12 replays over three rotating views (tests/test_gpu_view_bind.py's run, parameter updates
    between them) against view_cache=False; invalidate_views / an edited geometry tensor before replay
    6: the next visits are misses, whose plans are saved and hit again."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g, views = _gaussians(), _views()
    l0, s0, _ = _run(g, views, SEQ, 3, wait, at=6, what=what, view_cache=False)
    lb, sb, pb = _run(g, views, SEQ, 3, wait, at=6, what=what)
    assert pb.bound and pb._views.bind
    torch.testing.assert_close(lb, l0, rtol=1e-5, atol=0)
    assert_states_close(sb, s0, f"plans vs uncached, {what}, wait={wait}")
    st = pb.view_cache_stats()
    assert st["hits"] >= (2 if what else 4) and st["drops"] == (1 if what else 0), st
    packs = list(pb._views.packs.values())
    assert packs and all(v[3] == _native.view_plan_pack_bytes(1500, 70, 50, v[1]) for v in packs)
    # the run ends on hits: the sets' tables name plans
    words = _plan_words(pb)
    assert set(words) <= {0, PLAN_ON} and any(words), words
    if what is None:
        assert words == [PLAN_ON] * 3, words


def test_fixed_view_two_sets_on_one_pack(monkeypatch):
    """No slots and two sets (bench.py's form): one key, both sets bound to the one pack with its plan."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g = _gaussians()
    cam, gt, mask = _views(1)[0]
    bg = torch.zeros(3, device=DEV)

    def run(**kw):
        m = _frozen_model(g)
        opt = _adam(m)
        pg = PipelinedGraphStep(lambda: render(cam, m, _Pipe, bg, _Opt, language_target=(gt, mask))["language_l1"],
                                [m._language_feature], opt, model=m, sets=2, **kw)
        pg.capture()
        losses = []
        for _ in range(8):
            losses.append(pg.replay().clone())
            torch.cuda.synchronize()
        assert pg.check()
        pg.sync()
        return torch.stack(losses), _state(m, opt), pg

    l0, s0, _ = run(view_cache=False)
    l1, s1, pg = run()
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    assert_states_close(s1, s0, "fixed view, two sets")
    st = pg.view_cache_stats()
    assert st["packs"] == 1 and st["hits"] >= 5, st
    (pack,) = [v[2] for v in pg._views.packs.values()]
    assert all(b is pack for b in pg._views.bound) and len(pg._views.bound) == 2
    assert _plan_words(pg) == [PLAN_ON] * 2
