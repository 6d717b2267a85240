"""Device buffers carved out of sentinel-filled allocations (test helper, not a test module).

Every tensor a kernel writes in the branch / tail / limit tests comes from Arena.new(): a view
into a larger uint8 allocation pre-filled with SENTINEL, with at least GUARD elements of it on
each side.  Arena.check() compares both guards with the sentinel as integers, so a ragged tail
that writes one element too far (or one vector too early) fails the test instead of landing in
a neighbouring allocation.  off_bytes shifts the view off its 16-byte alignment, to steer the
kernels' alignment dispatch."""
import numpy as np
import torch

SENTINEL = 0xA5
GUARD = 64


class Arena:
    def __init__(self, device="cuda"):
        self.device = device
        self._items = []

    def new(self, shape, dtype, off_bytes=0, init=None, guard=GUARD):
        """A contiguous `shape` tensor of `dtype` whose first byte lies off_bytes past a 16-byte
        boundary, initialised from `init` (array / tensor / scalar; None leaves the sentinel)."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        es = torch.empty((), dtype=dtype).element_size()
        assert off_bytes % es == 0 and 0 <= off_bytes < 16
        nbytes = int(np.prod(shape, dtype=np.int64)) * es
        lead = (guard * es + 15) // 16 * 16 + off_bytes
        tail = guard * es + 16
        raw = torch.full((lead + nbytes + tail,), SENTINEL, dtype=torch.uint8, device=self.device)
        assert raw.data_ptr() % 16 == 0
        t = raw[lead:lead + nbytes].view(dtype).view(shape)
        assert t.data_ptr() % 16 == off_bytes and t.is_contiguous()
        if init is not None:
            if isinstance(init, np.ndarray):
                init = torch.from_numpy(np.ascontiguousarray(init))
            if torch.is_tensor(init):
                t.copy_(init.to(dtype).reshape(shape))
            else:
                t.fill_(init)
        self._items.append((raw, lead, nbytes))
        return t

    def check(self):
        """Both guards of every tensor handed out still hold the sentinel."""
        torch.cuda.synchronize()
        for k, (raw, lead, nbytes) in enumerate(self._items):
            lo, hi = raw[:lead], raw[lead + nbytes:]
            assert int((lo != SENTINEL).sum()) == 0, f"buffer {k}: bytes written before its start"
            assert int((hi != SENTINEL).sum()) == 0, f"buffer {k}: bytes written past its end"
