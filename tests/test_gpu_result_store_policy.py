"""Result stores of the forward render family: every store form writes the same bits, only there, and every kind of consumer sees them.

The forward kernels leave their result through several store forms -- 16- and 8-byte vectors behind a scalar plane address or behind a per-lane
64-bit address, element-aligned vectors, the 8-pixel kernels' piece exchange, the repeat-inner kernel's store_at, the batch kernel's closing
stores -- and the cache policy of those stores is a measured choice (profiles/EXPERIMENTS.md, "Forward kernel: result-store policy": plain,
the streaming hint, device-scope write-through, or both; one policy per kernel family, one of them picked per launch).  Whatever the policy,
each row below must hold:
  * the result is torch.equal to the same call forced onto the one-pixel kernels (tuning={"max_vec": 1}: plain scalar stores), NaN fringe of
    the allocation included -- the project asserts bit-equality across pixels-per-lane everywhere;
  * a torch kernel on the same stream, a torch kernel on a second stream behind an event, `.cpu()`, and two replays of a captured graph with the
    albedo changed in between all read those bits.
Shapes are the smallest at which a store path can go wrong; each case pins the kernel it ran (plan.kernel_name)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

G = 256                      # guard elements per side of a result (1 KiB: keeps the 16-byte alignment the 8-pixel kernels ask for)
NAN = float("nan")
VIEW = [0.1, -0.2, 1.0]


def _maps(B, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    albedo = torch.rand(B, 3, H, W, generator=g)
    normal = torch.nn.functional.normalize(torch.rand(B, 3, H, W, generator=g) * 2 - 1 + torch.tensor([0.0, 0.0, 1.5]).view(1, 3, 1, 1), dim=1)
    rough = torch.rand(B, 1, H, W, generator=g) * 0.95 + 0.05
    metal = torch.rand(B, 1, H, W, generator=g)
    return [t.to(dtype).cuda() for t in (albedo, normal * 0.5 + 0.5, rough, metal)]


def _lights(n):
    if n == 1:
        return [0.1, 0.1, 1.0], [1.0, 1.0, 1.0]
    pos = [[math.cos(2 * math.pi * i / n), math.sin(2 * math.pi * i / n), 1.0] for i in range(n)]
    return pos, [[1.0 / n, 0.8 / n, 0.6 / n]] * n


class Result:
    """A [B,3,H,W] result inside a NaN-filled allocation, `lead` elements further in than the guard (lead = 1: element-aligned vectors)."""

    def __init__(self, B, H, W, dtype=torch.float32, lead=0):
        n = B * 3 * H * W
        self.buf = torch.full((n + 2 * G + lead,), NAN, dtype=dtype, device="cuda")
        self.out = self.buf[G + lead:G + lead + n].view(B, 3, H, W)

    def refill(self):
        self.buf.fill_(NAN)


def _same(got, want, tag):
    """Whole allocations, bit for bit: the written values, and the NaN fringe where nothing may be written."""
    got, want = got.float().cpu(), want.float().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (tag, "written outside the result, or a value not written")
    assert torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0)), (tag, "values differ from the one-pixel kernels'")


#         id                  B  H  W   maps           lights  light_type     tile  lead  kernel of the rules     (what it exercises)
CASES = [("ragged_3x4",       1, 3, 4,  torch.float32, 1, "point",       1, 0, "ct_point_metallic_f32_f32_v4"),    # one lane per row
         ("ragged_2x5",       1, 2, 5,  torch.float32, 1, "point",       1, 0, "ct_point_metallic_f32_f32_v4"),    # the last two lanes of a row overlap: same pixels stored twice
         ("rows_5x33",        1, 5, 33, torch.float32, 1, "point",       1, 0, "ct_point_metallic_f32_f32_v4"),    # several tile rows, ragged
         ("f16_2x16",         1, 2, 16, torch.float16, 1, "point",       1, 0, "ct_point_metallic_f16_f32_v8"),    # 8-pixel lanes, the piece exchange
         ("f16_3x24",         1, 3, 24, torch.float16, 1, "point",       1, 0, "ct_point_metallic_f16_f32_v8"),    # ... with a partial last tile
         ("one_pixel_2x3",    1, 2, 3,  torch.float32, 1, "point",       1, 0, "ct_point_metallic_f32_f32_v1"),    # one-pixel kernels: untouched
         ("batch2_3x8",       2, 3, 8,  torch.float32, 1, "point",       1, 0, "ct_point_metallic_f32_f32_v4"),    # a tile crosses materials: per-lane 64-bit addresses
         ("repeat_point",     1, 4, 8,  torch.float32, 1, "point",       2, 0, "ctr_point_metallic_f32_f32_v4"),   # repeat-inner store_at, one evaluation per repeat
         ("repeat_dir",       1, 4, 8,  torch.float32, 1, "directional", 2, 0, "ctr_directional_metallic_f32_f32_v4"),   # ... one evaluation stored at every repeat
         ("offset_view_3x8",  1, 3, 8,  torch.float32, 1, "point",       1, 1, "ct_point_metallic_f32_f32_v4"),    # `out` starts one element into its allocation
         ("batch_kernel",     4, 2, 8,  torch.float16, 16, "point",      1, 0, "ctb_point_metallic_f16_f32_v2_b"),  # the batch kernel's closing stores
         # one material, rows of whole 256-pixel tiles, planes 64 MiB apart (a small view of a large allocation: the launcher reads the
         # stride): the launch runs the linear workgroup order and the one-light fp32 kernel's stores write through (ct_launch.hpp:
         # result_stores_through) -- behind a scalar plane address, behind per-lane 64-bit addresses (scalar_base = 0), element-aligned
         ("linear_2x256",     1, 2, 256, torch.float32, 1, "point",      1, 0, "ct_point_metallic_f32_f32_v4"),
         ("linear_nosb_3x256", 1, 3, 256, torch.float32, 1, "directional", 1, 0, "ct_directional_metallic_f32_f32_v4"),
         ("linear_off_3x512", 1, 3, 512, torch.float32, 1, "point",      1, 1, "ct_point_metallic_f32_f32_v4")]
PLANE = 1 << 24              # elements between the albedo planes of the `linear_` rows (64 MiB)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_result_stores_match_one_pixel_kernels_for_every_consumer(case):
    from pypbr_amd import functional as F
    name, B, H, W, dtype, n_lights, light_type, tile, lead, kernel = case
    maps = _maps(B, H, W, dtype, seed=len(name) * 131 + H * 17 + W)
    light, inten = _lights(n_lights)
    kw = dict(view_dir=VIEW, light=light, light_intensity=inten, light_type=light_type, light_size=1.0, tile=tile)
    tuning = None
    if name.startswith("linear_"):
        wide = torch.empty(3 * PLANE, dtype=dtype, device="cuda")          # never filled: only the view's H x W values per plane are touched
        view = wide.as_strided((B, 3, H, W), (3 * PLANE, PLANE, W, 1))
        view.copy_(maps[0])
        maps[0] = view
        tuning = {"scalar_base": 0} if "_nosb_" in name else None
    res, ref = Result(B, tile * H, tile * W, lead=lead), Result(B, tile * H, tile * W, lead=lead)
    plan = F.plan_cook_torrance(*maps, out=res.out, tuning=tuning, **kw)
    one = F.plan_cook_torrance(*maps, out=ref.out, tuning={"max_vec": 1}, **kw)
    assert plan.kernel_name.startswith(kernel), (name, plan.kernel_name)
    assert "_v1" in one.kernel_name and not one.kernel_name.startswith(("ctr_", "ctb_")), (name, one.kernel_name)
    if lead:
        assert res.out.data_ptr() % 16 == 4

    def reference():
        ref.refill()
        one.launch()
        torch.cuda.synchronize()
        return ref.buf.clone()

    want = reference()
    assert bool(torch.isfinite(ref.out).all()) and bool(torch.isnan(ref.buf[:G + lead]).all()) and bool(torch.isnan(ref.buf[G + lead + ref.out.numel():]).all())

    # a torch kernel on the same stream, nothing in between
    plan.launch()
    same_stream = res.buf.clone()
    # a torch kernel on a second stream behind an event
    res.refill()
    plan.launch()
    done = torch.cuda.Event()
    done.record()
    side = torch.cuda.Stream()
    side.wait_event(done)
    with torch.cuda.stream(side):
        second_stream = res.buf.clone()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    # the host
    res.refill()
    plan.launch()
    host = res.buf.cpu()
    _same(same_stream, want, (name, "same stream"))
    _same(second_stream, want, (name, "second stream"))
    _same(host, want, (name, ".cpu()"))

    # two replays of a captured graph (one stream, no parallel branches), the albedo changed in between
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    res.refill()
    with torch.cuda.graph(graph):
        plan.launch()
    for step in range(2):
        maps[0].mul_(0.5).add_(0.125 * (step + 1))
        res.refill()
        graph.replay()
        replayed = res.buf.clone()
        torch.cuda.synchronize()
        changed = reference()
        assert not torch.equal(torch.nan_to_num(changed, 7.0), torch.nan_to_num(want, 7.0)), (name, "the albedo edit changed nothing")
        _same(replayed, changed, (name, "graph replay %d" % step))
        want = changed
