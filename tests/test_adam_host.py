"""MaterialAdam without a device: the definition (tools/adam_oracle.py) against torch.optim.Adam in float64, its projections against torch's
clamp and F.normalize, the zero-update rule, the float16 rule, the ValueErrors of construction, the state dict's round trip with
torch.optim.Adam, the table entry's layout and the validation codes of pbr_adam_step / pbr_adam_advance (calls that launch nothing)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adam_oracle as A  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import optim  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial  # noqa: E402


def test_oracle_equals_torch_adam_in_float64_over_ten_steps_and_two_groups():
    rng = np.random.default_rng(11)
    shapes = [(3, 5, 7), (1, 5, 7)]
    options = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6)]
    p0 = [rng.uniform(-1, 1, s) for s in shapes]
    grads = [[rng.standard_normal(s) * 10.0 ** rng.uniform(-6, -1, s) for s in shapes] for _ in range(10)]
    params = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.Adam([dict(params=[q], **o) for q, o in zip(params, options)])
    state = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in p0]
    worst = 0.0
    for t, gs in enumerate(grads, start=1):
        for q, g in zip(params, gs):
            q.grad = torch.from_numpy(g.copy())
        opt.step()
        state = [A.step(p, g, m, v, t, **o) for (p, m, v), g, o in zip(state, gs, options)]
        for q, (p, m, v) in zip(params, state):
            worst = max(worst, float(np.abs(q.detach().numpy() - p).max()),
                        float(np.abs(opt.state[q]["exp_avg"].numpy() - m).max()), float(np.abs(opt.state[q]["exp_avg_sq"].numpy() - v).max()))
    print("float64 oracle against torch.optim.Adam after 10 steps: %.2e" % worst)
    assert worst <= 1e-12


def test_projections_equal_clamp_and_normalize_exactly():
    rng = np.random.default_rng(12)
    p = rng.uniform(-0.5, 1.5, (2, 3, 5, 7))
    t = torch.from_numpy(p)
    assert np.array_equal(A.project(p, bounds=(0.0, 1.0)), torch.clamp(t, 0.0, 1.0).numpy())
    assert np.array_equal(A.project(p, bounds=(0.05, None)), torch.clamp(t, min=0.05).numpy())
    assert np.array_equal(A.project(p, bounds=(None, 1.0)), torch.clamp(t, max=1.0).numpy())
    assert np.array_equal(A.project(p), p)
    want = t.clone()
    want[:, 2].clamp_(min=0.25)
    # F.normalize adds the squares in the order x, y, z with one rounding per product-and-sum: the oracle's fma(z, z, fma(y, y, x x)).
    # This pins how the host kernel of the torch build at hand forms the norm (2.10: vectorised fused multiply-adds); a build that sums
    # in another order would differ here in the last bit of some values with no defect in the product -- the definition is the chain.
    want = torch.nn.functional.normalize(want, dim=-3)
    got = A.project(p, "unit", min_z=0.25)
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(A.project(p[0], "unit"), torch.nn.functional.normalize(t[0], dim=-3).numpy())
    zero = np.zeros((3, 1, 2))
    assert np.array_equal(A.project(zero, "unit"), zero)                           # |p| below 1e-12: divided by 1e-12
    nan = np.array([np.nan, 2.0, -1.0]).reshape(1, 1, 3)
    assert np.isnan(A.project(nan, bounds=(0.0, 1.0))[0, 0, 0]) and np.array_equal(A.project(nan, bounds=(0.0, 1.0))[0, 0, 1:], [1.0, 0.0])
    with pytest.raises(ValueError):
        A.project(np.zeros((2, 4, 4)), "unit")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_update_keeps_the_bits(dtype):
    rng = np.random.default_rng(13)
    p = rng.uniform(-2.0, 2.0, (3, 4, 6)).astype(dtype)                            # outside every bound, not unit
    g = rng.standard_normal((3, 4, 6)).astype(dtype) * 1e-3
    g[:, 1:3, 2:5] = 0.0                                                           # pixels no shot covers
    g[0, 0, 0] = 0.0                                                               # one channel only: the pixel still moves as a whole under "unit"
    zeros = np.zeros_like(p)
    for kw in (dict(), dict(bounds=(0.0, 1.0)), dict(project_kind="unit", min_z=0.0)):
        q, m, v = A.step(p, g, zeros, zeros, 1, dtype=dtype, **kw)
        assert q.dtype == dtype and np.array_equal(q[:, 1:3, 2:5], p[:, 1:3, 2:5]) and (m[:, 1:3, 2:5] == 0).all() and (v[:, 1:3, 2:5] == 0).all()
        moved = np.ones(p.shape, bool)
        moved[:, 1:3, 2:5] = False
        if "project_kind" in kw:
            assert (q[:, moved[0]] != p[:, moved[0]]).all() and abs(np.sqrt((q[:, 0, 0] ** 2).sum()) - 1) < 1e-6
        else:
            moved[0, 0, 0] = False
            assert q[0, 0, 0] == p[0, 0, 0] and (q[moved] != p[moved]).all()
        if "bounds" in kw:
            assert q[moved].min() >= 0 and q[moved].max() <= 1


def test_float16_parameter_is_the_master_rounded():
    rng = np.random.default_rng(14)
    master = rng.uniform(0.0, 1.0, (1, 6, 8)).astype(np.float16).astype(np.float32)
    m, v = np.zeros_like(master), np.zeros_like(master)
    for t in range(1, 4):
        g = (rng.standard_normal(master.shape) * 1e-2).astype(np.float16)
        p16, master, m, v = A.step(master, g, m, v, t, lr=1e-3, bounds=(0.0, 1.0), dtype=np.float32, half=True)
        assert p16.dtype == np.float16 and master.dtype == np.float32 and m.dtype == np.float32 and v.dtype == np.float32
        assert np.array_equal(p16, master.astype(np.float16))
    assert not np.array_equal(master, p16.astype(np.float32))                      # the master holds what float16 cannot


def test_construction_errors():
    w = torch.zeros(3, 4, 4, requires_grad=True)
    one = torch.zeros(1, 4, 4, requires_grad=True)
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError):
            optim.MaterialAdam([w], **kw)
        with pytest.raises(ValueError):
            optim.MaterialAdam([dict(params=[w], **kw)])
    with pytest.raises(ValueError):
        optim.MaterialAdam([dict(params=[one], project="unit")])                   # channels != 3
    with pytest.raises(ValueError):
        optim.MaterialAdam([dict(params=[torch.zeros(2, 4, 4, 4, requires_grad=True)], project="unit")])
    with pytest.raises(ValueError):
        optim.MaterialAdam([dict(params=[w], bounds=(1.0, 0.0))])                  # lo > hi
    with pytest.raises(ValueError):
        optim.MaterialAdam([dict(params=[w], project="sphere")])
    opt = optim.MaterialAdam([dict(params=[w], project="unit", min_z=0.1), dict(params=[one], bounds=(None, 1.0))], lr=1e-2)
    assert opt.param_groups[0]["project"] == "unit" and opt.param_groups[1]["bounds"] == (None, 1.0) and opt.param_groups[1]["lr"] == 1e-2
    with pytest.raises(ValueError):
        opt.add_param_group(dict(params=[torch.zeros(2, 2, requires_grad=True)], project="unit"))
    # the lr schedulers work on it
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    assert sched.get_last_lr() == [1e-2, 1e-2]
    # no CPU path: a parameter that is not on a ROCm device raises at step()
    w.grad = torch.ones_like(w)
    with pytest.raises(RuntimeError):
        opt.step()


def test_material_param_groups():
    g = torch.Generator().manual_seed(3)
    n = torch.nn.functional.normalize(torch.rand(3, 4, 6, generator=g) + torch.tensor([-0.5, -0.5, 1.0])[:, None, None], dim=0)
    mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 4, 6, generator=g), roughness=torch.rand(1, 4, 6, generator=g),
                                    metallic=torch.rand(1, 4, 6, generator=g))
    mat.__dict__["_store"]["normal"] = n                                           # (decoding a normal map needs the device: filed as decoded)
    groups = optim.material_param_groups(mat, lr=1e-2, lr_normal=1e-3, roughness_min=0.08, min_z=0.1)
    by = {name: grp for name, grp in zip(("albedo", "normal", "roughness", "metallic"), groups)}
    store = mat.__dict__["_store"]
    assert all(grp["params"][0] is store[name] and store[name].requires_grad for name, grp in by.items())
    assert by["albedo"]["bounds"] == (0.0, 1.0) and by["metallic"]["bounds"] == (0.0, 1.0) and by["roughness"]["bounds"] == (0.08, 1.0)
    assert by["normal"]["project"] == "unit" and by["normal"]["min_z"] == 0.1 and by["normal"]["lr"] == 1e-3 and by["albedo"]["lr"] == 1e-2
    only = optim.material_param_groups(mat, maps=["roughness"])
    assert len(only) == 1 and only[0]["bounds"] == (0.05, 1.0)
    optim.MaterialAdam(groups)                                                     # the groups construct
    with pytest.raises(ValueError):
        optim.material_param_groups(mat, maps=["height"])


def test_state_dict_round_trip_with_torch_adam():
    rng = np.random.default_rng(15)
    p0 = rng.uniform(0.2, 0.8, (3, 4, 5))
    grads = [rng.standard_normal(p0.shape) * 1e-2 for _ in range(5)]

    def run(opt, q, gs):
        for g in gs:
            q.grad = torch.from_numpy(g.copy())
            opt.step()
    a = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    adam = torch.optim.Adam([a], lr=1e-2, betas=(0.85, 0.99), eps=1e-7)
    run(adam, a, grads[:3])
    mine = optim.MaterialAdam([dict(params=[torch.tensor(p0, dtype=torch.float64, requires_grad=True)], bounds=(0.0, 1.0))])
    mine.load_state_dict(copy.deepcopy(adam.state_dict()))                                  # torch.optim.Adam -> MaterialAdam
    group = mine.param_groups[0]
    assert group["lr"] == 1e-2 and group["betas"] == (0.85, 0.99) and group["eps"] == 1e-7 and group["bounds"] == (0.0, 1.0) and group["project"] is None
    st = mine.state[group["params"][0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3 and st["exp_avg"].shape == a.shape
    # (deep copies: load_state_dict keeps the tensors it is given, and two optimisers on one exp_avg would both move it)
    assert torch.equal(st["exp_avg"], adam.state[a]["exp_avg"]) and torch.equal(st["exp_avg_sq"], adam.state[a]["exp_avg_sq"])
    b = a.detach().clone().requires_grad_(True)
    back = torch.optim.Adam([b], lr=1.0)
    back.load_state_dict(copy.deepcopy(mine.state_dict()))                                  # MaterialAdam -> torch.optim.Adam: it steps on
    assert back.param_groups[0]["lr"] == 1e-2 and back.param_groups[0]["betas"] == (0.85, 0.99)
    run(adam, a, grads[3:])
    run(back, b, grads[3:])
    assert torch.equal(a, b) and float(back.state[b]["step"]) == 5
    # the oracle continues from the loaded state as torch.optim.Adam does
    p, m, v = a.detach().numpy(), adam.state[a]["exp_avg"].numpy(), adam.state[a]["exp_avg_sq"].numpy()
    q = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    ref = torch.optim.Adam([q], lr=1e-2, betas=(0.85, 0.99), eps=1e-7)
    run(ref, q, grads[:4])
    p4, m4, v4 = A.step(q.detach().numpy(), grads[4], ref.state[q]["exp_avg"].numpy(), ref.state[q]["exp_avg_sq"].numpy(), 5, lr=1e-2,
                        betas=(0.85, 0.99), eps=1e-7)
    assert np.abs(p4 - p).max() <= 1e-12 and np.abs(m4 - m).max() <= 1e-12 and np.abs(v4 - v).max() <= 1e-12


def test_table_entry_layout():
    lib = N.lib()
    assert lib.pbr_adam_tensor_size() == ctypes.sizeof(N.AdamTensor) == 112
    assert ctypes.sizeof(N.AdamCoeffs) == 24 and ctypes.sizeof(N.AdamGroup) == 48
    header = abi_header.RAW
    assert "#define PBR_MAX_ADAM_TENSORS %d" % N.MAX_ADAM_TENSORS in header and N.MAX_ADAM_TENSORS >= 8
    assert "#define PBR_ADAM_BLOCK %d " % N.ADAM_BLOCK in header and "#define PBR_ADAM_MAX_BLOCKS %d " % N.ADAM_MAX_BLOCKS in header
    assert "PBR_ADAM_NONE = %d, PBR_ADAM_BOX = %d, PBR_ADAM_UNIT = %d" % (N.ADAM_NONE, N.ADAM_BOX, N.ADAM_UNIT) in header


BASE = 1 << 20          # addresses that are never dereferenced: every call below returns before anything is launched


def _entry(**kw):
    f = dict(param=BASE, grad=2 * BASE, exp_avg=3 * BASE, exp_avg_sq=4 * BASE, master=None, pixels=64, param_batch_stride=192,
             param_plane_stride=64, grad_batch_stride=192, grad_plane_stride=64, batch=1, channels=3, dtype=N.F32, project=N.ADAM_NONE,
             lo=0.0, hi=1.0, min_z=0.0, group=0)
    f.update(kw)
    return N.AdamTensor(*[f[name] for name, _ in N.AdamTensor._fields_])


def _step(entries, n=None, host=True, device=None, n_groups=1, null_table=False):
    table = (N.AdamTensor * len(entries))(*entries)
    coeffs = (N.AdamCoeffs * N.MAX_ADAM_TENSORS)() if host else None
    return N.lib().pbr_adam_step(None if null_table else table, len(entries) if n is None else n, coeffs, device, n_groups, None)


def test_adam_step_validation_codes():
    ok = _entry()
    assert _step([ok], null_table=True) == N.ERR_NULL_MAP
    assert _step([ok], host=False) == N.ERR_NULL_MAP                               # neither coefficient table
    assert _step([ok], device=5 * BASE) == N.ERR_NULL_MAP                          # both
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert _step([_entry(**{name: None})]) == N.ERR_NULL_MAP, name
    assert _step([_entry(dtype=N.F16)]) == N.ERR_NULL_MAP                          # float16 without its master
    assert _step([_entry(master=5 * BASE)]) == N.ERR_UNSUPPORTED                   # a master behind float32
    assert _step([ok], n=0) == N.ERR_SHAPE and _step([ok], n=N.MAX_ADAM_TENSORS + 1) == N.ERR_SHAPE
    assert _step([ok], n_groups=0) == N.ERR_SHAPE and _step([ok], n_groups=N.MAX_ADAM_TENSORS + 1) == N.ERR_SHAPE
    assert _step([_entry(group=1)]) == N.ERR_SHAPE and _step([_entry(group=-1)]) == N.ERR_SHAPE
    for name in ("batch", "channels", "pixels"):
        assert _step([_entry(**{name: 0})]) == N.ERR_SHAPE, name
    for name in ("param_batch_stride", "param_plane_stride", "grad_batch_stride", "grad_plane_stride"):
        assert _step([_entry(**{name: -64})]) == N.ERR_SHAPE, name
    assert _step([_entry(param_plane_stride=63)]) == N.ERR_SHAPE                   # written planes on top of each other
    assert _step([_entry(batch=2, param_batch_stride=191)]) == N.ERR_SHAPE         # ... images
    assert _step([_entry(dtype=7)]) == N.ERR_DTYPE
    assert _step([_entry(project=3)]) == N.ERR_UNSUPPORTED
    assert _step([_entry(project=N.ADAM_UNIT, channels=1)]) == N.ERR_CHANNELS
    assert _step([_entry(project=N.ADAM_UNIT, channels=4, param_batch_stride=256, grad_batch_stride=256)]) == N.ERR_CHANNELS
    assert _step([_entry(project=N.ADAM_BOX, lo=1.0, hi=0.5)]) == N.ERR_SHAPE
    assert _step([_entry(param=BASE + 2)]) == N.ERR_SHAPE                          # off the element's alignment
    assert _step([_entry(exp_avg=3 * BASE + 2)]) == N.ERR_SHAPE
    # in-place-illegal overlaps: the gradient on the parameter, state on state, two entries on one parameter
    assert _step([_entry(grad=BASE)]) == N.ERR_SHAPE
    assert _step([_entry(grad=BASE + 4 * 191)]) == N.ERR_SHAPE                     # by one element
    assert _step([_entry(exp_avg_sq=3 * BASE + 4 * 100)]) == N.ERR_SHAPE
    assert _step([ok, _entry(grad=6 * BASE, exp_avg=7 * BASE, exp_avg_sq=8 * BASE)]) == N.ERR_SHAPE
    assert _step([ok, _entry(param=6 * BASE, grad=3 * BASE, exp_avg=7 * BASE, exp_avg_sq=8 * BASE)]) == N.ERR_SHAPE   # reads what entry 0 writes
    assert N.error_string(N.ERR_CHANNELS)


def test_interleaved_maps_of_a_material_major_packing_are_accepted_up_to_the_launch():
    """pack_maps(material_major=True), B = 2: material 0's normal lies between material 0's and material 1's albedo, so the first-to-last
    spans of the maps intersect while no element is shared.  pbr_adam_check -- what pbr_adam_step checks before it launches, alone --
    accepts the four maps of such a packing in one table and refuses the same table with one map moved an element into its neighbour
    (tests/test_gpu_adam.py steps the accepted layout on the device)."""
    hw = 64
    pitch = 8 * hw                                                                 # albedo 3 + normal 3 + roughness 1 + metallic 1 planes per material

    def packed(offset, channels, k, **kw):
        return _entry(param=BASE + 4 * offset, grad=2 * BASE + 4 * offset, exp_avg=(3 + 3 * k) * BASE, exp_avg_sq=(4 + 3 * k) * BASE, pixels=hw, batch=2,
                      channels=channels, param_batch_stride=pitch, param_plane_stride=hw, grad_batch_stride=pitch, grad_plane_stride=hw, **kw)
    maps = [packed(0, 3, 0), packed(3 * hw, 3, 1, project=N.ADAM_UNIT), packed(6 * hw, 1, 2), packed(7 * hw, 1, 3)]
    # one element into the neighbour's plane: refused, in every position of the packing
    for k, off in ((1, 3 * hw - 1), (2, 6 * hw - 1), (3, 7 * hw - 1), (3, 7 * hw + 1)):
        bad = list(maps)
        bad[k] = packed(off, maps[k].channels, k, project=maps[k].project)
        assert _step(bad) == N.ERR_SHAPE, (k, off)
        assert N.lib().pbr_adam_check((N.AdamTensor * 4)(*bad), 4, 1) == N.ERR_SHAPE
    assert N.lib().pbr_adam_check((N.AdamTensor * 4)(*maps), 4, 1) == N.OK
    assert N.lib().pbr_adam_check((N.AdamTensor * 4)(*maps), 4, 0) == N.ERR_SHAPE and N.lib().pbr_adam_check(None, 4, 1) == N.ERR_NULL_MAP
    # an expanded gradient (stride 0) repeats its plane: reads may overlap themselves, never something written
    assert N.lib().pbr_adam_check((N.AdamTensor * 1)(_entry(grad_plane_stride=0, grad_batch_stride=0)), 1, 1) == N.OK
    assert N.lib().pbr_adam_check((N.AdamTensor * 1)(_entry(grad=BASE + 4 * 64, grad_plane_stride=0, grad_batch_stride=0)), 1, 1) == N.ERR_SHAPE


def test_adam_advance_validation_codes():
    rows = (N.AdamGroup * 2)(N.AdamGroup(BASE, None, 1e-3, 0.9, 0.999, 1e-8), N.AdamGroup(None, None, 1e-3, 0.9, 0.999, 1e-8))
    lib = N.lib()
    assert lib.pbr_adam_advance(None, 1, 2 * BASE, None) == N.ERR_NULL_MAP
    assert lib.pbr_adam_advance(rows, 1, None, None) == N.ERR_NULL_MAP
    assert lib.pbr_adam_advance(rows, 2, 2 * BASE, None) == N.ERR_NULL_MAP         # a row without its counter
    assert lib.pbr_adam_advance(rows, 0, 2 * BASE, None) == N.ERR_SHAPE
    assert lib.pbr_adam_advance(rows, N.MAX_ADAM_TENSORS + 1, 2 * BASE, None) == N.ERR_SHAPE
