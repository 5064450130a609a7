"""`Context`: the one Python owner of a context of the C library (include/samaudio.h) - its handle, the tensors the library borrows
from it and its scratch - for the engine contexts (model.py, judge.py) and every tower (`samaudio_<tower>_*`); `scratch`, the one rule
by which a scratch buffer is sized, poisoned and aligned; `check_keys`, the strict-mode bookkeeping of the towers' load_state_dict."""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import hip


def check_keys(want, have, strict: bool) -> Tuple[List[str], List[str]]:
    """(missing, unexpected) of a state dict with the keys `have` against the keys `want`, sorted; `strict` raises on either, with
    torch.nn.Module.load_state_dict's exception type."""
    missing, unexpected = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    if strict and (missing or unexpected):
        raise RuntimeError(f"Missing keys: {missing}, unexpected_keys: {unexpected}")
    return missing, unexpected


def _aligned(buf: torch.Tensor) -> Tuple[C.c_void_p, int]:
    """(pointer rounded up to 256, bytes of `buf` behind it)"""
    base = buf.data_ptr()
    aligned = (base + 255) // 256 * 256
    return C.c_void_p(aligned), buf.numel() - (aligned - base)


def scratch(owner, attr: str, need: int, device) -> Tuple[C.c_void_p, int]:
    """The scratch buffer `owner.<attr>` (uint8, or None) grown to hold `need` bytes behind a 256-byte aligned pointer, which is
    returned with the bytes behind it.  It takes the owner and not the buffer because the old block is released BEFORE the new one is
    allocated (the two need not fit side by side), which takes dropping the owner's reference.
    SAMAUDIO_POISON (tests/conftest.py sets it) fills a new buffer with SAMAUDIO_POISON_BYTE, default 0xFF = NaN in fp32 and bf16: a
    kernel that reads scratch nobody wrote then shows up as NaN deterministically instead of depending on what the allocator handed
    out; a finite pattern (e.g. 0x3F) shows the reads that NaN-ignoring ops hide."""
    buf = getattr(owner, attr)
    if buf is None or buf.numel() < need + 256:
        buf = None
        setattr(owner, attr, None)
        if os.environ.get("SAMAUDIO_POISON"):
            fill = int(os.environ.get("SAMAUDIO_POISON_BYTE", "255"), 0)
            buf = torch.full((need + 256,), fill, dtype=torch.uint8, device=device)
        else:
            buf = torch.empty(need + 256, dtype=torch.uint8, device=device)
        setattr(owner, attr, buf)
    return _aligned(buf)


class Context:
    """One context of the library's `abi` family ("samaudio", "samaudio_judge", ...): `<abi>_create` here, `<abi>_destroy` in close().
    `_h` is the raw handle (what `lib.<abi>_*` take), `_tensors` the registered tensors it keeps alive, `_workspace` its scratch
    (None: the next ensure_workspace allocates a fresh one), `_loaded` whether finalize() went through."""

    def __init__(self, lib, abi: str, config, *, device=None, operands: Optional[str] = None,
                 alt16: Optional[Callable[[str], bool]] = None):
        """`operands`, `alt16(name)`: what hip.dtype_code checks 16-bit tensors against (the DiT engine contexts pass them)"""
        self._lib, self._abi, self.device = lib, abi, device
        self._operands, self._alt16 = operands, alt16
        self._tensors: Dict[str, torch.Tensor] = {}
        self._workspace: Optional[torch.Tensor] = None
        self._loaded = False
        self._h = C.c_void_p()
        hip.check(self._fn("create")(C.byref(config), C.byref(self._h)))

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._abi}_{name}")

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None   # (getattr: __init__ may have raised before there was a handle)
        if h:
            getattr(self._lib, self._abi + "_destroy")(h)

    __del__ = close

    def set_option(self, option: int, value: int) -> None:
        hip.check(self._fn("set_option")(self._h, option, value))

    def finalize(self, *what: int) -> None:
        hip.check(self._fn("finalize")(self._h, *what))
        self._loaded = True

    def register(self, tensors: Dict[str, torch.Tensor], borrowed: bool = False) -> None:
        """`<abi>_set_tensor` of every tensor.  The library borrows the pointers: each tensor is kept alive in `_tensors`, a view
        into a larger buffer that is not 16-byte aligned as a clone.  `borrowed`: another context keeps these very tensors alive
        (a stream lane's, a side context's weights) - nothing is cloned or stored."""
        set_tensor = self._fn("set_tensor")
        for name, t in tensors.items():
            dt = hip.dtype_code(t.dtype, self._operands, alt_ok=self._alt16 is not None and self._alt16(name))
            if borrowed:
                assert t.data_ptr() % 16 == 0, f"{name}: a borrowed tensor must be 16-byte aligned"
            else:
                if t.data_ptr() % 16:
                    t = t.clone()
                self._tensors[name] = t
            hip.check(set_tensor(self._h, name.encode(), hip.ptr(t), dt, t.dim(), hip.shape_array(t.shape)))

    def ensure_workspace(self, *shape: int) -> None:
        """a workspace of `<abi>_workspace_bytes(*shape)` bytes (see scratch), handed to the library"""
        need = self._fn("workspace_bytes")(self._h, *shape)
        hip.check(self._fn("set_workspace")(self._h, *scratch(self, "_workspace", need, self.device)))

    def lend_workspace(self, other: "Context", *shape: int) -> None:
        """hand `other` this context's workspace as it is, for a call of `other` with `shape` (stream order keeps the two apart)"""
        ptr, usable = _aligned(self._workspace)
        need = other._fn("workspace_bytes")(other._h, *shape)
        assert usable >= need, f"a borrowed workspace of {usable} bytes, {need} needed"
        hip.check(other._fn("set_workspace")(other._h, ptr, usable))
