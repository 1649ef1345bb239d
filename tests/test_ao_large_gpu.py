"""Ambient occlusion (include/rt_capi_ao.h) over records that pass 2^32 bytes, by the conventions of test_large_extents_gpu.py: one
launch over the 4.31 GB of records of a 9 472 x 9 472 depth-0 G-buffer rendered on the device, its output between sentinel guards,
compared on the device word for word with the same kernel run over chunks of at most 1 024 columns (each chunk's records at offset
0 of its own launch, key0 = x0 * H), and columns 0, 4 735 and 9 471 against ao_ref.  Bit-exact."""
import numpy as np
import pytest

import ao_ref
import large_extents as le
import oracle_lib as oracle
import query_ref
from large_extents import Guarded
from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu
F = np.float32
SIDE, R, SEED = 9472, 2.0, 1


def test_ao_of_records_past_2_32_bytes():
    import torch
    W = H = SIDE
    cw, hw = 3 * H, 12 * H                                     # words per column: colours, records
    assert hw * W * 4 > (1 << 32) and (hw * 4) % 16 == 0
    need = Guarded.need(hw * W) + cw * W * 4 + Guarded.need(H * W) + Guarded.need(le.STRIP_COLUMNS * H) + (3 << 30)
    le.require_device_memory(need)
    r, hits, out, rgb = Renderer(HostScene.builtin()), None, None, None
    what = f"rt_ambient_occlusion_device over the records of {W}x{H}"
    try:
        hits, out = Guarded(hw * W), Guarded(H * W)
        rgb = torch.empty((cw * W,), dtype=torch.float32, device="cuda")
        r.render_gbuffer_device(W, H, 0, 0, W, rgb.data_ptr(), hits.ptr)
        r.ambient_occlusion_device(W * H, H, hits.ptr, out.ptr, samples=1, radius=R, seed=SEED)
        assert r.kernel_name() == "rt_ao_kernel"
        torch.cuda.synchronize()
        hits.assert_written(what + ": the records")
        out.assert_written(what)
        before = le.checksum(hits.body)

        def chunk(x0, x1, ptr):
            r.ambient_occlusion_device((x1 - x0) * H, H, hits.ptr + x0 * hw * 4, ptr, samples=1, radius=R, seed=SEED, key0=x0 * H)

        le.assert_columns_equal_strips(chunk, [(out.body, H)], W, what)
        assert le.checksum(hits.body) == before and hits.guards_untouched(), "the records are only read"
        o = oracle.OracleScene.builtin()
        scene, cam = query_ref.Scene(o), HostScene.builtin().camera
        seen = set()
        for x in (0, 4735, 9471):
            records = query_ref.intersect(scene, le.column_rays(cam, W, H, x, x + 1))
            want = ao_ref.ambient_occlusion(scene, records, 1, R, seed=SEED, key0=x * H)
            got = out.body[x * H:(x + 1) * H].cpu().numpy().view(F)
            d = le.first_difference(got.view(np.int32), want.reshape(-1).view(np.int32))
            assert d is None, f"{what}: column {x} against ao_ref: {d[3]} values differ, first at row {d[0]}"
            seen |= set(np.unique(want).tolist())
        assert seen == {0.0, 1.0}                              # (one direction a record: closed or open, and both occur)
        assert out.guards_untouched()
    finally:
        for g in (hits, out):
            if g is not None:
                g.free()
        del rgb
        r.close()
        torch.cuda.empty_cache()
