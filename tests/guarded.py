"""Guarded device buffers and the smallest accepted workspace, for the tests of the memory contract of include/smx.h.

A plain helper module (imported by name; no fixtures): tests/test_gpu_memory_contract.py and tests/test_gpu_memory_entries.py
hand every buffer of a call to the library inside a Guarded and check afterwards that nothing outside the stated extent was
written; tests/test_guarded_cpu.py proves on CPU tensors that the checker sees damage; tests/test_agg_workspace.py takes its
bisection from here, so the size the host test accepts and the size the kernels run in cannot drift apart.
"""
import ctypes as C

import numpy as np

SMX_E_WS = -3
ALIGN = 256          # what the library aligns the caller's workspace up to (smx_agg.hip align_up)


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64,
            np.dtype(np.uint64): torch.int64}[np.dtype(dtype)]


class Guarded:
    """One torch.uint8 allocation `front guard | payload | back guard`, all of it filled with `fill`.

    nbytes / dtype / shape: the payload (dtype a numpy dtype, nbytes == prod(shape) * itemsize); it starts `misalign` bytes
    past a 256-byte boundary.  plane: w*h of the call the buffer belongs to -- each guard is at least
    max(4096, 4 * plane rounded up to 4096) bytes, so that a stray row or plane still lands inside this allocation.
    .view: the typed payload tensor;  .ptr: its address as a c_void_p."""

    def __init__(self, nbytes, dtype, shape, misalign=0, fill=0xA5, plane=0, device="cuda"):
        import torch
        dtype = np.dtype(dtype)
        assert nbytes == int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, (nbytes, dtype, shape)
        assert 0 <= misalign < ALIGN and misalign % dtype.itemsize == 0, (misalign, dtype)
        self.nbytes, self.fill, self.misalign = int(nbytes), int(fill), int(misalign)
        guard = max(4096, (4 * int(plane) + 4095) // 4096 * 4096)
        self.buf = torch.full((guard + ALIGN + misalign + self.nbytes + guard,), self.fill, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        # the first address >= base + guard that lies `misalign` bytes past a 256-byte boundary
        self.front = (base + guard - misalign + ALIGN - 1) // ALIGN * ALIGN + misalign - base
        self.bytes = self.buf[self.front:self.front + self.nbytes]
        self.view = self.bytes.view(_torch_dtype(dtype)).view(*shape) if self.nbytes else self.bytes
        self.content = None
        assert (base + self.front) % ALIGN == misalign and self.front >= guard
        assert self.buf.numel() - self.front - self.nbytes >= guard

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.front)

    def load(self, array):
        """Copy `array` (numpy, the payload's size) into the payload and remember it: check_unchanged compares with it."""
        import torch
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        self.content = torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
        self.bytes.copy_(self.content)
        return self

    def numpy(self):
        return self.view.cpu().numpy()

    def _sync(self):
        if self.buf.is_cuda:
            import torch
            torch.cuda.synchronize(self.buf.device)

    def damage(self):
        """None, or (first, last): the offsets, relative to the payload's first byte, of the first and the last guard byte
        that no longer holds `fill` (negative in the front guard, >= nbytes in the back guard)."""
        self._sync()
        bad = []
        for lo, hi in ((0, self.front), (self.front + self.nbytes, self.buf.numel())):
            idx = (self.buf[lo:hi] != self.fill).nonzero()
            if idx.numel():
                bad += [lo + int(idx[0]) - self.front, lo + int(idx[-1]) - self.front]
        return (bad[0], bad[-1]) if bad else None

    def check(self, name):
        """Synchronise, then every guard byte still holds `fill`."""
        d = self.damage()
        assert d is None, (f"{name}: written outside its {self.nbytes} bytes (payload {self.misalign} B past a 256-byte "
                           f"boundary): first damaged byte at offset {d[0]}, last at {d[1]}")

    def check_unchanged(self, name):
        """check(), and the payload still holds what load() put there (an input of the call)."""
        self.check(name)
        assert self.content is not None
        idx = (self.bytes.cpu() != self.content).nonzero()
        assert idx.numel() == 0, f"{name}: an input was modified, first at byte {int(idx[0])}, last at {int(idx[-1])}"

    def check_untouched(self, name):
        """check(), and the payload still holds `fill` everywhere (a call that must not have launched anything)."""
        self.check(name)
        idx = (self.bytes != self.fill).nonzero()
        assert idx.numel() == 0, f"{name}: written although nothing ran, first at byte {int(idx[0])}, last at {int(idx[-1])}"


def agg_chunk(so, p, w, h, nviews, cost, own_q, forced, ws, n):
    """smx_debug_agg_chunk: (chunk, 0) or (None, error code) of a call on a workspace of `ws` bytes of which the worst case
    of 255 are lost to the 256-byte alignment of the caller's pointer."""
    out = C.c_int()
    rc = so.smx_debug_agg_chunk(C.byref(p), w, h, nviews, cost, own_q, forced, ws, n, C.byref(out))
    return (out.value, 0) if rc == 0 else (None, rc)


def min_workspace(so, p, w, h, nviews, cost, own_q, forced, n):
    """The smallest workspace, in 256-byte steps, that a call of n slices with these arguments accepts (smx_debug_agg_chunk,
    with the 255 lost bytes built in): bisection between 0, which fails, and nviews x smx_agg_workspace_bytes(w, h, 1), which
    include/smx.h promises to be enough for any call."""
    args = (p, w, h, nviews, cost, own_q, forced)
    lo, hi = 0, nviews * so.smx_agg_workspace_bytes(w, h, 1) // 256            # lo fails, hi holds
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if agg_chunk(so, *args, mid * 256, n)[1] == 0 else (mid, hi)
    return hi * 256


def hooks(so_path, params_type):
    """The library with the debug hooks and the workspace sizes typed (they are not part of include/smx.h's bound set)."""
    L = C.CDLL(so_path)
    L.smx_debug_agg_chunk.restype = C.c_int
    L.smx_debug_agg_chunk.argtypes = [C.POINTER(params_type), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_uint64, C.c_int, C.POINTER(C.c_int)]
    L.smx_debug_agg_path.restype = C.c_int
    L.smx_debug_agg_path.argtypes = [C.POINTER(params_type), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.smx_agg_workspace_bytes.restype = C.c_size_t
    L.smx_agg_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.smx_agg_workspace_bytes_for.restype = C.c_size_t
    L.smx_agg_workspace_bytes_for.argtypes = [C.POINTER(params_type), C.c_int, C.c_int, C.c_int]
    return L
