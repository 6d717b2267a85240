"""Minibatch row gather and uint8 widening (csrc/gather.hip) on every copy width, stride and loop.

ppox_gather_rows copies in uint4, uint32 or byte lanes by the row size, the row stride and both base
pointers' alignment; its grid covers at most 8192 rows per trip.  Reference: the rollout indexed as
buffer.py:41-52 does after swap_and_flatten, obs[idx % T, idx // T] (torch's own indexing, on the device).
Destinations are carved out of sentinel-filled buffers (tests/guarded.py)."""
import numpy as np
import pytest
import torch

from guarded import Arena

pytestmark = pytest.mark.gpu

T, N = 5, 7

# (row_bytes, padding of the padded source stride, dst offsets from a 16-byte boundary)
WIDTHS = [(16, 16, (0, 4, 1)),  # uint4; dst 4 bytes off: uint32 lanes, 1 byte off: bytes
          (28_224, 16, (0,)),  # a frame stack: more vectors than threads
          (20, 4, (0,)),  # uint32 lanes
          (7, 1, (0,)),  # bytes
          (1, 1, (0,))]
CASES = [(rb, pad, off) for rb, p, offs in WIDTHS for pad in (0, p) for off in offs]


@pytest.mark.parametrize("nrows", [1, 8193])
@pytest.mark.parametrize("row_bytes,pad,dst_off", CASES)
def test_gather_rows_widths_strides_and_row_loop(row_bytes, pad, dst_off, nrows):
    import native
    stride = row_bytes + pad
    g = torch.Generator(device="cuda").manual_seed(row_bytes * 31 + pad + dst_off + nrows)
    src = torch.randint(0, 256, (T, N, stride), dtype=torch.uint8, device="cuda", generator=g)
    idx = torch.randint(0, T * N, (nrows,), device="cuda", generator=g)
    idx[-1] = T * N - 1
    if nrows > 1:
        idx[0] = 0
    ar = Arena()
    dst = ar.new((nrows, row_bytes), torch.uint8, off_bytes=dst_off)
    native.gather_rows(src, T, N, row_bytes, stride, idx, nrows, dst)
    ar.check()
    assert torch.equal(dst, src[idx % T, idx // T, :row_bytes])


def test_gather_rows_no_rows_is_ok():
    import native
    src = torch.zeros(T, N, 16, dtype=torch.uint8, device="cuda")
    native.gather_rows(src, T, N, 16, 16, torch.empty(0, dtype=torch.int64, device="cuda"), 0,
                       torch.empty(0, 16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


def test_u8_to_f32_grid_stride():
    """(8192 * 256 + 5) * 16 bytes: five lanes past one trip of the 8192-block grid."""
    import native
    n = (8192 * 256 + 5) * 16
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    ar = Arena()
    out = ar.new(n, torch.float32)
    native.u8_to_f32(x, out=out)
    ar.check()
    assert torch.equal(out, x.float())
    got = out[-80:].cpu().numpy()
    assert np.array_equal(got, x[-80:].cpu().numpy().astype(np.float32))


def test_u8_to_f32_empty_and_ragged():
    import native
    out = native.u8_to_f32(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert out.numel() == 0 and out.dtype == torch.float32
    x = torch.zeros(24, dtype=torch.uint8, device="cuda")
    ar = Arena()
    dst = ar.new(24, torch.float32)
    with pytest.raises(native.NativeError, match="multiple of 16"):
        native.u8_to_f32(x, out=dst)
    ar.check()
    assert (dst.view(torch.int32) == -0x5A5A5A5B).all()  # untouched: still the sentinel bytes
