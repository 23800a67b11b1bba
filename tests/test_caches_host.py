"""CPU-only checks of pypbr_amd._caches -- what the host-side caches share: the identity predicate, the parameter snapshot, the
tensor-keyed memo, the kept plan -- and of what rests on it: the empty-output launch of a kept plan and a material's invalidation."""
import gc
import weakref

import pytest
import torch

from pypbr_amd import _caches as C
from pypbr_amd import functional as F
from pypbr_amd.materials import BasecolorMetallicMaterial


def test_settings_are_shared_with_functional():
    assert F.CACHING is C.CACHING and F.set_caching is C.set_caching and F.version_of is C.version_of
    assert C.CACHING == {"device_maps": False, "parameters": False, "decode_verdicts": False}


def test_same_tensors_is_about_objects_not_values():
    a, b = torch.ones(3), torch.zeros(2)
    refs = C.weak_refs((a, None, b))
    assert refs[1] is None and C.same_tensors(refs, (a, None, b))
    assert not C.same_tensors(refs, (a.clone(), None, b))             # equal values, another object
    assert not C.same_tensors(refs, (a, b, b)) and not C.same_tensors(refs, (None, None, b))      # None against a tensor, either way
    assert not C.same_tensors(refs, (a, None))                        # fewer tensors than were held
    del b
    gc.collect()
    assert refs[2]() is None and not C.same_tensors(refs, (a, None, torch.zeros(2)))


def test_host_values_snapshots_host_parameters_only():
    assert C.host_values(torch.tensor([0.0, 0.5, 1.0])) == [0.0, 0.5, 1.0]
    nested = [[0.1, 0.2, 1.0], (0.0, 0.0, 1.0)]
    snap = C.host_values(nested)
    assert snap == [[0.1, 0.2, 1.0], [0.0, 0.0, 1.0]]
    nested[0][0] = 9.0
    nested.append([1.0, 1.0, 1.0])
    assert snap == [[0.1, 0.2, 1.0], [0.0, 0.0, 1.0]]
    flat = [0.0, 0.0, 1.0]
    snap = C.host_values(flat)
    flat[2] = 2.0
    assert snap == [0.0, 0.0, 1.0]
    assert C.host_values(torch.ones(3, requires_grad=True)) is None
    assert C.host_values(1.0) is None and C.host_values(None) is None


def test_version_memo():
    memo = C.VersionMemo()
    t = torch.zeros(3)
    payload = object()
    assert memo.get(t, C.version_of(t)) is None and len(memo) == 0
    memo.put(t, C.version_of(t), payload)
    assert memo.get(t, C.version_of(t)) is payload and len(memo) == 1
    t.add_(1)                                                         # an in-place edit bumps the version counter
    assert memo.get(t, C.version_of(t)) is None
    # another tensor that reuses a freed id: the entry's weak reference is dead, or refers to another object
    old = id(t)
    ver = C.version_of(t)
    memo.put(t, ver, payload)
    del t
    gc.collect()
    other = torch.zeros(3)
    memo._entries[id(other)] = memo._entries.pop(old)
    assert memo.get(other, ver) is None
    live = torch.ones(2)
    memo._entries[id(other)] = memo._entries[id(live)] = (weakref.ref(live), 0, payload)
    assert memo.get(live, 0) is payload and memo.get(other, 0) is None
    memo.clear()
    assert len(memo) == 0
    with torch.inference_mode():
        assert C.version_of(torch.zeros(3)) is None


def test_version_memo_sweeps_dead_entries_and_clears_at_its_limit():
    memo = C.VersionMemo(limit=3)
    a, b, c, d = (torch.zeros(1) for _ in range(4))
    memo.put(a, 0, "a")
    memo.put(b, 0, "b")
    del a
    gc.collect()
    assert len(memo) == 2                                             # swept on put, not before
    memo.put(c, 0, "c")
    assert len(memo) == 2 and memo.get(b, 0) == "b" and memo.get(c, 0) == "c"
    memo.put(d, 0, "d")
    assert len(memo) == 3
    e = torch.zeros(1)
    memo.put(e, 0, "e")                                               # at the limit: everything is forgotten first
    assert len(memo) == 1 and memo.get(e, 0) == "e" and memo.get(b, 0) is None


PARAMS = ([0.0, 0.0, 1.0], [0.1, 0.1, 1.0], [1.0, 1.0, 1.0])


def _plan(out=None, params=PARAMS):
    """A RenderPlan over CPU tensors (the descriptor is pure host logic), its maps in the plan's order and their host values."""
    B, H, W = (2, 8, 16) if out is None else (out.shape[0], out.shape[2], out.shape[3])
    maps = (torch.rand(B, 3, H, W), torch.rand(B, 3, H, W), torch.rand(B, 1, H, W), torch.rand(B, 1, H, W), None)
    out = torch.empty(B, 3, H, W) if out is None else out
    d = F.build_descriptor(*maps, out, view_dir=params[0], light=params[1], light_intensity=params[2], light_type="point", light_size=None,
                           albedo_is_srgb=True, specular_is_srgb=True, return_srgb=True, convert_to_diffuse_specular=False, y_offset=0,
                           height_total=None)
    return F.RenderPlan(d, out, maps, False), maps, tuple(C.host_values(p) for p in params)


def test_kept_plan_adopts_only_plans_that_point_into_the_callers_tensors():
    plan, maps, vals = _plan()
    kept = C.KeptPlan.adopt(plan, maps, vals, (2, 3, 8, 16))
    assert kept is not None and plan._keep == () and kept.plan is plan and kept.values == vals and kept.out_shape == (2, 3, 8, 16)
    assert not hasattr(kept, "__dict__")
    plan, maps, vals = _plan()
    staged = maps[:2] + (maps[2].clone(),) + maps[3:]                 # one kept tensor is a copy: another address
    plan._keep = staged
    assert C.KeptPlan.adopt(plan, maps, vals) is None and plan._keep is staged
    plan, maps, vals = _plan()
    plan._param_block = torch.zeros(4)
    assert C.KeptPlan.adopt(plan, maps, vals) is None and plan._keep is maps


def test_kept_plan_describes_refreshes_and_locks():
    plan, maps, vals = _plan()
    kept = C.KeptPlan.adopt(plan, maps, vals)
    assert kept.out_shape is None and kept.describes(maps)
    assert not kept.describes(maps[:3] + (maps[3].clone(), None))     # one map replaced
    d = plan.desc
    before = bytes(d)
    assert kept.refresh(tuple(C.host_values(p) for p in PARAMS)) and bytes(d) == before and kept.values is vals
    edited = (vals[0], [-0.3, 0.1, 1.0], vals[2])
    assert kept.refresh(edited) and kept.values is edited
    assert [d.lights[0][c] for c in range(3)] == pytest.approx([-0.3, 0.1, 1.0]) and bytes(d) != before
    before = bytes(d)
    two = (vals[0], [[0.1, 0.1, 1.0], [-0.3, 0.2, 0.8]], vals[2])
    assert not kept.refresh(two) and kept.values is edited and bytes(d) == before and d.n_lights == 1
    assert kept.try_acquire() and not kept.try_acquire()
    kept.release()
    assert kept.try_acquire()
    kept.release()


def test_a_kept_plan_launches_an_empty_output_without_the_library():
    plan, maps, _ = _plan(out=torch.empty(1, 3, 0, 16))
    assert maps[3] is not None                                        # a metallic map was given

    def library_call(*args):
        pytest.fail("an empty result needs no launch")
    plan._fn = library_call
    plan._keep = ()                                                   # what KeptPlan.adopt leaves behind
    assert plan.launch(stream=0) is plan.out and plan.out.shape == (1, 3, 0, 16)


def test_a_materials_call_caches_do_not_travel_with_copies():
    mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 4, 4), roughness=torch.rand(1, 4, 4), metallic=torch.rand(1, 4, 4))
    dummies = {"_device_cache": object(), "_plan_cache": object(), "_plan_seen": object()}
    mat.__dict__.update(dummies)
    for copy in (mat.clone(), mat._shallow()):
        assert not any(k in copy.__dict__ for k in dummies)
    assert all(mat.__dict__[k] is v for k, v in dummies.items())      # the original keeps its own
    assert mat.drop_device_cache() is mat
    assert "_device_cache" not in mat.__dict__ and "_plan_cache" in mat.__dict__ and "_plan_seen" in mat.__dict__
