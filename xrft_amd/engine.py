"""Thin object wrapper over the C ABI: one ``SpectralPlan`` = one ``xrfthip_plan`` + its workspace.

torch is used only as the owner of device memory and the provider of the current HIP stream; every
arithmetic step runs inside libxrft_hip.so.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib

_HALF = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}  # real half-precision INPUT of a plan (the float32 plan reading 2-byte samples) and of convert(); nothing else takes it
_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.complex64: _lib.C64, torch.complex128: _lib.C128}
_REAL_OF = {torch.float32: torch.float32, torch.float64: torch.float64, torch.complex64: torch.float32,
            torch.complex128: torch.float64, torch.float16: torch.float32, torch.bfloat16: torch.float32}
_CPLX_OF = {torch.float32: torch.complex64, torch.float64: torch.complex128, torch.complex64: torch.complex64,
            torch.complex128: torch.complex128, torch.float16: torch.complex64, torch.bfloat16: torch.complex64}


def _stream_handle(t):
    if t.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class SpectralPlan:
    """detrend -> window -> (flip, ifftshift) -> FFT over the last ``ndim`` axes -> shift/phase/scale ->
    complex | power | cross (-> radial bin-sum), in one call on the current stream."""

    def __init__(self, ndim, batch, ny, nx, dtype, out_mode=_lib.OUT_COMPLEX, detrend=_lib.DETREND_NONE, flags=0,
                 scale=1.0, window_y=None, window_x=None, phase_y=None, phase_x=None, binmap=None, nbins=0,
                 slabs_per_group=0, inner=1, mid=1, in_stride_y=0, in_stride_batch=0, herm_ny=0, herm_nx=0, phase_hx=None, mean_batch=0, seg_hop=0, seg_stride=0, seg_keep=0, seg_synth=0,
                 seg_filter=0, seg_lead=0, seg_in_len=0, seg_out_len=0, seg_tapers=0, seg_taper_len=0, tapers=None, seg_filter_cols=0):
        self._dll = _lib.load()
        self._h = C.c_void_p(0)
        self._serial = next(_PLAN_SERIAL)  # who produced a pass-1 block (an id() can come back after the plan has gone)
        self._pass1 = None
        if dtype not in _DTYPES and dtype not in _HALF:
            raise TypeError(f"unsupported dtype {dtype}")
        self.ndim, self.batch, self.ny, self.nx = int(ndim), int(batch), int(ny), int(nx)
        self.dtype, self.out_mode, self.flags = dtype, int(out_mode), int(flags)
        half_y = (bool(flags & _lib.HALF_X) and bool(flags & _lib.AXIS_Y)) or bool(flags & _lib.HALF_Y)  # (ABI 0.1.4: real_dim along the ONE transformed axis of an AXIS_Y plan; 0.1.6: HALF_Y of the inner / mid layouts)
        self.nx_out = self.nx // 2 + 1 if ((flags & _lib.HALF_X) and not half_y) else self.nx
        self.ny_out = self.ny // 2 + 1 if half_y else self.ny
        self.nbins = int(nbins)
        self.inner = max(int(inner), 1)  # > 1: (batch, ny, nx, inner) arrays, the transform axes are not the trailing ones
        self.mid = max(int(mid), 1)      # > 1: (batch, ny, mid, nx, inner): independent elements between the two transform axes
        # input strides in elements (0 = dense): the plan reads a box of a larger array where it lies (xrfthip_desc.in_stride_y / in_stride_batch)
        self.in_stride_y, self.in_stride_batch = int(in_stride_y), int(in_stride_batch)
        # the last pass of a three-axis spectrum (xrfthip_desc.herm_ny / herm_nx): (batch, nt, herm_ny, herm_nx/2 + 1) complex in, the full (batch, nt, herm_ny, herm_nx) out;
        # with HERM_FIELD the complex transform itself (out_mode COMPLEX), whose output-phase tables are phase_y (t), phase_x (herm_ny) and phase_hx (herm_nx, the full axis)
        self.herm_ny, self.herm_nx = int(herm_ny), int(herm_nx)
        if self.herm_ny or self.herm_nx:
            self.nx_out = self.herm_ny * self.herm_nx
        # the mean over every ``mean_batch`` consecutive slabs inside the last pass (xrfthip_desc.mean_batch): batch // M outputs; 0 | 1 = the plain plan
        self.mean_batch = int(mean_batch)
        self.batch_out = self.batch // self.mean_batch if self.mean_batch > 1 else self.batch
        # Welch spectra (xrfthip_desc.seg_hop): the mean_batch segments of nx samples of each series start seg_hop samples apart; in_stride_batch is the series pitch
        self.seg_hop = int(seg_hop)
        # ... along a leading axis (xrfthip_desc.seg_stride): ``inner`` adjacent series whose samples lie seg_stride elements apart, blocks in_stride_batch apart;
        # the result is (blocks, inner, nx_out).  1 (with inner = 1) says what the rows layout says
        self.seg_stride = int(seg_stride)
        # every segment's spectrum kept (xrfthip_desc.seg_keep): mean_batch counts the segments of a series (1 is allowed), nothing is averaged; the result is
        # (series, mean_batch, nx_out), or (blocks, mean_batch, nx_out, inner) in the column layout
        self.seg_keep = int(seg_keep)
        if self.seg_keep:
            self.batch_out = self.batch // max(self.mean_batch, 1)
        # the series rebuilt from its segments' half spectra (xrfthip_desc.seg_synth; complex64, INVERSE | C2R_X): mean_batch counts the segments of a series, the input
        # is (series, mean_batch, nx / 2 + 1) -- in_stride_batch the pitch between series in complex elements -- and the result (series, (mean_batch - 1) seg_hop + nx), real
        self.seg_synth = int(seg_synth)
        if self.seg_synth:
            self.batch_out = self.batch // max(self.mean_batch, 1)
        # a series filtered by overlap-save (xrfthip_desc.seg_filter; float32, flags 0): nx = L the segment length, seg_hop = V the samples kept of each, mean_batch =
        # ceil(seg_out_len / V) the segments of a series; the input is (series, seg_in_len) -- in_stride_batch the pitch between series in samples -- and the result
        # (series, seg_out_len), real float32, from sample seg_lead of the full convolution; phase_x carries the response, nx / 2 + 1 entries
        self.seg_filter, self.seg_lead, self.seg_in_len, self.seg_out_len = int(seg_filter), int(seg_lead), int(seg_in_len), int(seg_out_len)
        if self.seg_filter:
            self.batch_out = self.batch // max(self.mean_batch, 1)
        # ... along a leading axis (xrfthip_desc.seg_filter_cols, with seg_stride = S >= inner): the input is the (blocks, seg_in_len, inner) view the plan addresses --
        # columns adjacent, samples S apart, blocks in_stride_batch apart -- and the result (blocks, seg_out_len, inner), the array's own order
        self.seg_filter_cols = int(seg_filter_cols)
        # multitaper spectra (xrfthip_desc.seg_tapers; float32, POWER | CROSS, seg_hop 0): nx = L the transform length, the input (series, seg_taper_len) -- in_stride_batch
        # the pitch between series in samples -- and the result (series, nx_out); ``tapers`` is the (seg_tapers, seg_taper_len) table, already weighted by sqrt(w_j)
        self.seg_tapers, self.seg_taper_len = int(seg_tapers), int(seg_taper_len)
        d = _lib.DescFiltCols(C.sizeof(_lib.DescFiltCols), self.ndim, self.batch, self.ny, self.nx, _HALF[dtype] if dtype in _HALF else _DTYPES[dtype], self.out_mode,
                      int(detrend), self.flags, float(scale), int(slabs_per_group), 0, self.inner, self.mid, self.in_stride_y, self.in_stride_batch,
                      self.herm_ny, self.herm_nx, self.mean_batch, self.seg_hop, 0, self.seg_stride, 0, self.seg_keep, 0, self.seg_synth, 0,
                      self.seg_filter, self.seg_lead, self.seg_in_len, self.seg_out_len, self.seg_tapers, self.seg_taper_len, self.seg_filter_cols, 0)
        _lib.check(self._dll.xrfthip_plan_create(C.byref(self._h), C.byref(d)))
        if tapers is not None:
            tp = np.ascontiguousarray(tapers, dtype=np.float32)
            if tp.shape != (self.seg_tapers, self.seg_taper_len):
                raise ValueError(f"taper table shape {tp.shape} != {(self.seg_tapers, self.seg_taper_len)}")
            _lib.check(self._dll.xrfthip_plan_set_tapers(self._h, tp.ctypes.data_as(C.c_void_p)))
        for axis, w in ((0, window_y), (1, window_x)):
            if w is not None:
                w = np.ascontiguousarray(w, dtype=np.float64)
                _lib.check(self._dll.xrfthip_plan_set_window(self._h, axis, w.ctypes.data_as(C.c_void_p), w.size))
        for axis, p in ((0, phase_y), (1, phase_x), (2, phase_hx)):
            if p is not None:
                p = np.ascontiguousarray(p, dtype=np.complex128)
                _lib.check(self._dll.xrfthip_plan_set_phase(self._h, axis, p.ctypes.data_as(C.c_void_p), p.size))
        if flags & _lib.ISO:
            bm = np.ascontiguousarray(binmap, dtype=np.int32)
            if bm.shape != (self.ny, self.nx_out):
                raise ValueError(f"bin map shape {bm.shape} != {(self.ny, self.nx_out)}")
            _lib.check(self._dll.xrfthip_plan_set_binmap(self._h, bm.ctypes.data_as(C.c_void_p), self.ny,
                                                         self.nx_out, self.nbins))

    def __del__(self):
        try:
            if self._h:
                self._dll.xrfthip_plan_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return int(self._dll.xrfthip_workspace_bytes(self._h))

    def describe(self):
        buf = C.create_string_buffer(8192)
        self._dll.xrfthip_plan_describe(self._h, buf, len(buf))
        return buf.value.decode()

    def kernel_info(self):
        """(kernel kind, independent sequences per workgroup) of the plan: ``_lib.K_*`` -- what ``describe()`` prints, as numbers."""
        k, n = C.c_int32(0), C.c_int32(0)
        _lib.check(self._dll.xrfthip_plan_kernel_info(self._h, C.byref(k), C.byref(n)))
        return int(k.value), int(n.value)

    def uses_bluestein(self):
        """True when an axis of the plan runs Bluestein's algorithm inside the tile kernels (a prime factor with no butterfly)."""
        return bool(self._dll.xrfthip_plan_uses_bluestein(self._h))

    def pass1(self):
        """(bytes of one field's pass-1 block, its signature per field) -- xrfthip_plan_pass1_bytes / _signature; (0, ()) where the plan hands no block over."""
        if self._pass1 is None:
            nb = int(self._dll.xrfthip_plan_pass1_bytes(self._h))
            sigs = []
            for f in range((2 if self.out_mode in (_lib.OUT_CROSS, _lib.OUT_PHASE, _lib.OUT_COHERENCE) else 1) if nb else 0):
                sig = C.c_uint64(0)
                _lib.check(self._dll.xrfthip_plan_pass1_signature(self._h, f, C.byref(sig)))
                sigs.append(int(sig.value))
            self._pass1 = (nb if sigs else 0, tuple(sigs))
        return self._pass1

    def set_profiling(self, enable=True):
        _lib.check(self._dll.xrfthip_plan_set_profiling(self._h, int(bool(enable))))

    def read_profile(self):
        """{label: (launches, total_ms)} from HIP events recorded around every launch since set_profiling(True)."""
        buf = C.create_string_buffer(1 << 16)
        n = self._dll.xrfthip_plan_profile_read(self._h, buf, len(buf))
        if n < 0:
            _lib.check(n)
        out = {}
        for line in buf.value.decode().splitlines():
            label, cnt, ms = line.rsplit(" ", 2)
            out[label] = (int(cnt), float(ms))
        return out

    def out_dtype(self):
        real = self.out_mode in (_lib.OUT_POWER, _lib.OUT_PHASE, _lib.OUT_COHERENCE) or (self.flags & _lib.C2R_X) or self.seg_filter  # (the filtered series is real)
        return _REAL_OF[self.dtype] if real else _CPLX_OF[self.dtype]

    def _layout_ok(self, t):
        """Does the memory layout of ``t`` match the plan's: contiguous, or -- a plan with input strides -- a view (..., ny, nx) whose last stride is 1, whose row
        stride is the plan's, whose leading dims collapse to ONE batch stride equal to the plan's, and whose first element is 16-byte aligned."""
        if self.seg_hop and self.seg_synth:  # (series, segments, bins): the half spectra adjacent, the segments of a series adjacent, the series the plan's pitch apart
            nb = self.nx // 2 + 1
            return (t.dim() == 3 and tuple(t.shape) == (self.batch_out, self.mean_batch, nb) and (t.stride(2) == 1 or nb == 1) and (t.stride(1) == nb or self.mean_batch == 1)
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or self.mean_batch * nb)))
        if self.seg_hop and self.seg_filter and self.seg_filter_cols:  # (blocks, samples, columns): exactly the view the plan addresses, seg_in_len samples a column
            return (t.dim() == 3 and tuple(t.shape) == (self.batch_out, self.seg_in_len, self.inner) and (self.inner <= 1 or t.stride(2) == 1)
                    and (self.seg_in_len <= 1 or t.stride(1) == self.seg_stride)
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or self.seg_in_len * self.seg_stride)))
        if self.seg_hop and self.seg_filter:  # (series, samples): exactly seg_in_len samples a series, adjacent, the series the plan's pitch apart
            return (t.dim() == 2 and tuple(t.shape) == (self.batch_out, self.seg_in_len) and (t.stride(1) == 1 or self.seg_in_len == 1)
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or self.seg_in_len)))
        if self.seg_tapers:  # (series, samples): exactly seg_taper_len samples a series, adjacent, the series the plan's pitch apart; 4-byte alignment is the dtype's
            return (t.dim() == 2 and tuple(t.shape) == (self.batch, self.seg_taper_len) and (t.stride(1) == 1 or self.seg_taper_len == 1)
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or self.seg_taper_len)))
        if self.seg_hop and self.seg_stride > 1:  # (blocks, samples, columns): exactly the view the plan addresses -- columns adjacent, samples seg_stride apart, blocks the plan's pitch apart
            span = (self.mean_batch - 1) * self.seg_hop + self.nx
            return (t.dim() == 3 and t.shape[0] == self.batch_out and t.shape[1] >= span and t.shape[2] == self.inner
                    and (self.inner <= 1 or t.stride(2) == 1) and t.stride(1) == self.seg_stride
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or span * self.seg_stride)))
        if self.seg_hop:  # (series, samples): rows of at least the segments' span, the plan's pitch apart, samples adjacent; 4-byte alignment is the dtype's
            span = (self.mean_batch - 1) * self.seg_hop + self.nx
            return (t.dim() == 2 and t.shape[0] == self.batch_out and t.shape[1] >= span and t.stride(1) == 1
                    and (t.shape[0] <= 1 or t.stride(0) == (self.in_stride_batch or span)))
        if not (self.in_stride_y or self.in_stride_batch):
            return t.is_contiguous()
        sy, sb = strides_of(t, self.ndim)
        if sy is None or t.data_ptr() % 16:
            return False
        want_y = self.in_stride_y or self.nx
        want_b = self.in_stride_batch or self.ny * self.nx
        return (self.ndim == 1 or self.ny == 1 or sy == want_y) and (self.batch <= 1 or sb == want_b)

    def execute(self, in0, in1=None, out=None, iso=None, sources=None):
        """``in0``/``in1``: contiguous tensors of shape (batch, ny, nx) (any leading shape that flattens to it); a plan made with ``in_stride_y`` /
        ``in_stride_batch`` takes the view with exactly those strides instead (see ``strides_of``).  Returns (out, iso); either may be None depending on the flags.
        ``sources``: per field, the caller's OWN device tensor whose memory ``in0`` / ``in1`` is (not a copy made for this call), or None: only such fields
        take part in the reuse of the column pass (``reuse_column_pass``)."""
        dev = in0.device
        nx_in = self.nx // 2 + 1 if (self.flags & _lib.C2R_X) else self.nx
        if in0.dtype != self.dtype or not self._layout_ok(in0) or (not self.seg_hop and not self.seg_tapers and in0.numel() != self.batch * self.ny * nx_in * self.inner * self.mid):
            raise ValueError("in0 does not match the plan (dtype / contiguity / size)")
        if self.out_mode in (_lib.OUT_CROSS, _lib.OUT_PHASE, _lib.OUT_COHERENCE):
            if in1 is None or in1.dtype != self.dtype or not self._layout_ok(in1) or (not self.seg_hop and not self.seg_tapers and in1.numel() != in0.numel()):
                raise ValueError("in1 does not match the plan")
        want_out = not (self.flags & _lib.NO_SPECTRUM_OUT)
        if want_out and out is None:
            shape = (self.batch_out, self.ny_out, self.nx_out) + ((self.inner,) if self.inner > 1 else ())
            if self.seg_hop and self.seg_stride > 1:  # (the column layout of a Welch plan: frequency last)
                shape = (self.batch_out, self.inner, self.nx_out)
            if self.seg_hop and self.seg_keep:  # (every segment's spectrum: the segments where the time axis lay, the columns innermost)
                shape = (self.batch_out, self.mean_batch, self.nx_out) + ((self.inner,) if self.seg_stride > 1 else ())
            if self.seg_hop and self.seg_synth:  # (the series)
                shape = (self.batch_out, (self.mean_batch - 1) * self.seg_hop + self.nx)
            if self.seg_hop and self.seg_filter:  # (the filtered series; the column layout: where the time axis lay, the columns innermost)
                shape = (self.batch_out, self.seg_out_len) + ((self.inner,) if self.seg_filter_cols else ())
            if self.seg_tapers:  # (one spectrum per series)
                shape = (self.batch, self.nx_out)
            if self.mid > 1:
                shape = (self.batch, self.ny_out, self.mid, self.nx_out, self.inner)
            if self.herm_ny:
                shape = (self.batch, self.ny, self.herm_ny, self.herm_nx)
            out = torch.empty(shape, dtype=self.out_dtype(), device=dev)
        elif want_out:  # a caller's buffer (graph capture, composed passes): held to the plan before the device sees its pointer
            need = self.batch_out * self.ny_out * self.nx_out * self.inner * self.mid * (self.mean_batch if self.seg_keep else 1)
            if self.seg_hop and self.seg_synth:
                need = self.batch_out * ((self.mean_batch - 1) * self.seg_hop + self.nx)
            if self.seg_hop and self.seg_filter:
                need = self.batch_out * self.seg_out_len * (self.inner if self.seg_filter_cols else 1)
            if out.dtype != self.out_dtype() or not out.is_contiguous() or out.numel() != need or out.device != dev:
                raise ValueError(f"out does not match the plan (dtype {self.out_dtype()}, contiguous, {need} elements on {dev})")
        iso_dtype = torch.complex128 if self.out_mode == _lib.OUT_CROSS else torch.float64
        nspec = self.batch * self.inner * self.mid  # (an inner / mid layout: every element is a spectrum with radial sums of its own)
        if self.flags & _lib.ISO and iso is None:
            iso = torch.empty((nspec, self.nbins), device=dev, dtype=iso_dtype)
        elif self.flags & _lib.ISO:
            if iso.dtype != iso_dtype or not iso.is_contiguous() or iso.numel() != nspec * self.nbins or iso.device != dev:
                raise ValueError(f"iso does not match the plan (dtype {iso_dtype}, contiguous, {nspec * self.nbins} elements on {dev})")
        if self.batch == 0:  # nothing to transform: empty outputs, no device call
            return (out if want_out else None), iso
        stream = _stream_handle(in0)
        # The C plan is immutable after creation, so nothing plan-wide is locked: threads on different streams enqueue
        # concurrently.  Callers that share a stream share its scratch buffer: their enqueues (a short sequence of kernel
        # launches each) must not interleave, hence one lock per (device, stream).
        with _stream_lock(dev, stream):
            # grown (and the outgrown buffer retired) only HERE, under the stream's lock: no other thread is between its look-up and
            # its enqueue on this stream, so the event recorded at retirement really follows every use of the old buffer
            fields = (in0,) if in1 is None else (in0, in1)
            if _takes_part(dev, sources, len(fields)) and self.pass1()[0]:
                self._execute_blocks(dev, stream, fields, sources, out if want_out else None, iso)
            else:
                ws = _workspace(dev, stream, self.workspace_bytes)
                _blocks_overwritten((str(dev), stream.value), 0, self.workspace_bytes)
                _lib.check(self._dll.xrfthip_exec(self._h, _ptr(in0), _ptr(in1), _ptr(out if want_out else None), _ptr(iso),
                                                  _ptr(ws), ws.numel(), stream))
        return (out if want_out else None), iso

    def _execute_blocks(self, dev, stream, fields, sources, out, iso):
        """xrfthip_exec_ex with every field's pass 1 in a block in front of the plan's private part of the stream's scratch: read from the block another plan left for
        the same unchanged field (no column pass, no fit kernel), or written there for the calls that follow.  Called with _stream_lock(dev, stream) held."""
        key = (str(dev), stream.value)
        nb, sigs = self.pass1()
        nf = len(fields)
        private = self.workspace_bytes - nf * nb  # (every field in a block: xrfthip_exec_ex)
        tags = [(t.data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device), t._version, stream.value, sigs[f])
                for f, t in enumerate(fields)]
        ws = _WS.get(key)
        slack = 0 if dev.type == "cuda" else 255  # (the emulated device's memory is the host's: 64-byte aligned; the blocks start on the first 256-byte boundary)
        while True:
            st = _BLOCKS.setdefault(key, {"gen": 0, "slots": []})
            live = [s for s in st["slots"] if s["gen"] == st["gen"]]
            # a block is read only if every item of its tag matches, the field's tensor is the very object it was written from, and ANOTHER plan wrote it:
            # a call repeated on an unchanged array computes everything again
            used, matched = [], {}
            for f in range(nf):
                for s in live:
                    if (s["tag"] == tags[f] and s["ref"]() is sources[f] and s["producer"] != self._serial and s["bytes"] == nb
                            and not any(s is m for m in matched.values())):
                        matched[f] = s
                        used.append((s["off"], s["off"] + nb))
                        break
            offs, at = {}, 0
            for f in range(nf):  # the fields to compute: the lowest places the blocks read in this call leave free
                if f in matched:
                    offs[f] = matched[f]["off"]
                    continue
                while any(at < e and b < at + nb for b, e in used):
                    at = min(e for b, e in used if at < e and b < at + nb)
                offs[f] = at
                used.append((at, at + nb))
            end = max(e for _b, e in used)
            new = [(offs[f], offs[f] + nb) for f in range(nf) if f not in matched]
            # blocks of the same size this call neither reads nor writes (the other field of a pair): kept where the scratch has the room -- a call that reads a
            # block may also grow the scratch for it, by no more than its own private part
            keep = max([end] + [s["off"] + s["bytes"] for s in live if s["bytes"] == nb and not any(s is m for m in matched.values())
                                and not any(s["off"] < e and b < s["off"] + s["bytes"] for b, e in new)])
            have = ws.numel() - slack if ws is not None else 0
            if keep + private <= have or (matched and keep > end):
                want_bytes, start = keep + private, keep
            else:
                want_bytes, start = end + private, end
            if want_bytes > have:
                ws = _workspace(dev, stream, want_bytes + slack)  # (a new buffer: every block is gone with the old one -- lay the call out again)
                continue
            break
        _PEAK[key] = max(_PEAK.get(key, 0), want_bytes)
        for b, e in new + [(start, start + private)]:
            _blocks_overwritten(key, b, e)
        a = _lib.ExecArgs()
        a.struct_size = C.sizeof(_lib.ExecArgs)
        a.d_in0, a.d_in1 = fields[0].data_ptr(), (fields[1].data_ptr() if nf == 2 else None)
        a.d_out, a.d_iso = (out.data_ptr() if out is not None else None), (iso.data_ptr() if iso is not None else None)
        base = (ws.data_ptr() + 255) & ~255
        a.d_workspace, a.ws_bytes, a.stream = base + start, max(private, 0), stream.value
        for f in range(nf):
            a.field[f].pass1_block = base + offs[f]
            a.field[f].pass1_mode = _lib.PASS1_CONSUME if f in matched else _lib.PASS1_PRODUCE
        _lib.check(self._dll.xrfthip_exec_ex(self._h, C.byref(a)))
        for f in range(nf):
            if f not in matched:
                st["slots"].append({"off": offs[f], "bytes": nb, "gen": st["gen"], "tag": tags[f], "ref": weakref.ref(sources[f]), "producer": self._serial})


def strides_of(t, ndim):
    """(row stride, batch stride) in elements of a tensor whose last ``ndim`` dims are the transform axes, as xrfthip_desc.in_stride_y / in_stride_batch describe it:
    the last stride is 1 and the leading dims collapse to one batch stride (size-1 dims aside).  (None, None) when the view has no such description.  A batch
    of one reports the dense batch stride; a 1-D transform the row length as its row stride."""
    if t.dim() < ndim or t.stride(-1) != 1 and t.shape[-1] > 1:
        return None, None
    nx = t.shape[-1]
    ny = t.shape[-2] if ndim == 2 else 1
    sy = t.stride(-2) if (ndim == 2 and ny > 1) else nx
    lead = [(n, s) for n, s in zip(t.shape[:t.dim() - ndim], t.stride()[:t.dim() - ndim]) if n > 1]
    sb = None
    for n, s in reversed(lead):  # innermost leading dim first: each outer stride must be (extent x stride) of the dim inside it
        if sb is None:
            sb, span = s, n * s
        elif s != span:
            return None, None
        else:
            span = n * s
    if sb is None:
        sb = ny * sy
    if sy < nx or sb <= 0:
        return None, None
    return int(sy), int(sb)


_PLAN_SERIAL = itertools.count(1)

# Reuse of the column pass.  The spectra of one pair of fields are computed back to back (xrft.cross_spectrum(a, b), then xrft.isotropic_power_spectrum(a) and (b)),
# each call through a plan of its own that begins with the SAME column pass over the same field.  The stream's scratch therefore keeps up to two pass-1 blocks
# (include/xrft_hip.h, xrfthip_exec_ex) in front of the running plan's private part, each with a tag: the field (data_ptr, storage offset, shape, strides, dtype,
# device, tensor._version, the tensor object itself), the stream, the plan's pass-1 signature, the plan that wrote it, the generation of the scratch buffer.
# A later call reads a block only when all of it matches and another plan wrote it.  Whatever writes a block's bytes (any exec on the scratch that reaches them), a
# new scratch buffer and clear_plan_cache() drop the tags.
_BLOCKS = {}   # (device, stream) -> {"gen": generation of the scratch buffer, "slots": [block, ...]}
_PEAK = {}     # (device, stream) -> the most scratch bytes a call with blocks has asked for (bench scripts)
_REUSE = [True]
_CAPTURED = [False]


def reuse_column_pass(enable=None):
    """Switch the reuse of a field's column pass between spectral products (default on); ``reuse_column_pass(False)``: every call computes everything inside its
    own workspace.  The results are bit-identical either way.  Returns the setting."""
    if enable is not None:
        _REUSE[0] = bool(enable)
    return _REUSE[0]


def _takes_part(dev, sources, nf):
    if not _REUSE[0] or sources is None or len(sources) != nf or any(not isinstance(s, torch.Tensor) for s in sources):
        return False
    if dev.type == "cuda" and not _CAPTURED[0] and torch.cuda.is_current_stream_capturing():
        _CAPTURED[0] = True  # a captured graph writes the scratch again whenever it is replayed, unseen from here: no block is trusted any more (until clear_workspaces)
    return not _CAPTURED[0]


def _blocks_overwritten(key, begin, end):
    """Bytes [begin, end) of the stream's scratch are about to be written: the blocks they reach are gone."""
    st = _BLOCKS.get(key)
    if st and st["slots"]:
        st["slots"] = [s for s in st["slots"] if s["gen"] == st["gen"] and (s["off"] >= end or s["off"] + s["bytes"] <= begin)]


# One grow-only scratch buffer per (device, stream), shared by every plan: work on one stream is ordered, so plans never
# overlap in it; two streams never share scratch memory.  (A workspace per plan pinned several GB per cached plan.)
_WS = {}
_WS_LOCKS = {}
_WS_RETIRED = []  # (buffer, event) of outgrown buffers: kernels enqueued earlier may still be using them until the event has passed
_WS_LOCK = threading.Lock()


def _stream_lock(dev, stream):
    key = (str(dev), stream.value)
    with _WS_LOCK:
        lock = _WS_LOCKS.get(key)
        if lock is None:
            lock = _WS_LOCKS[key] = threading.Lock()
        return lock


def _workspace(dev, stream, nbytes):
    """The stream's scratch buffer, grown if needed.  Call with _stream_lock(dev, stream) held."""
    key = (str(dev), stream.value)
    with _WS_LOCK:
        # outgrown buffers go once the work that may still use them has finished (an event recorded on their stream when they retired)
        _WS_RETIRED[:] = [(b, ev) for b, ev in _WS_RETIRED if ev is not None and not ev.query()]
        ws = _WS.get(key)
        if ws is None or ws.numel() < nbytes:
            want = max(int(nbytes), 256)
            if ws is not None:
                want = max(want, int(1.5 * ws.numel()))  # geometric growth: a session whose plans grow step by step re-allocates O(log) times
                ev = None
                if dev.type == "cuda":
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(dev))
                    _WS_RETIRED.append((ws, ev))
            ws = _WS[key] = torch.empty(want, dtype=torch.uint8, device=dev)
            st = _BLOCKS.get(key)
            if st is not None:  # a new buffer: a new generation, no blocks
                st["gen"] += 1
                st["slots"] = []
        return ws


def clear_workspaces():
    """Release the shared scratch buffers (synchronises the devices first)."""
    with _WS_LOCK:
        if _WS or _WS_RETIRED:
            if _lib.device() == "cuda" and torch.cuda.is_available():
                torch.cuda.synchronize()
            _WS.clear()
            _WS_RETIRED.clear()
        _BLOCKS.clear()
        _PEAK.clear()
        _CAPTURED[0] = False


def detrend(x, ndim, kind):
    """Stand-alone detrend over the last ``ndim`` (1|2|3) axes of a contiguous tensor (xrft/detrend.py:11-138)."""
    dll = _lib.load()
    if x.dtype not in _DTYPES or not x.is_contiguous():
        raise ValueError("detrend needs a contiguous float/complex tensor")
    if ndim == 3:
        n0, n1, n2 = x.shape[-3:]
        batch = x.numel() // max(n0 * n1 * n2, 1)
        out = torch.empty_like(x)
        nws = int(dll.xrfthip_detrend_workspace_bytes(batch))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        _lib.check(dll.xrfthip_detrend3(_DTYPES[x.dtype], batch, n0, n1, n2, kind, _ptr(x), _ptr(out), _ptr(ws), nws,
                                        _stream_handle(x)))
        return out
    nx = x.shape[-1]
    ny = x.shape[-2] if ndim == 2 else 1
    batch = x.numel() // max(ny * nx, 1)
    out = torch.empty_like(x)
    nws = int(dll.xrfthip_detrend_workspace_bytes(batch))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    _lib.check(dll.xrfthip_detrend(_DTYPES[x.dtype], ndim, batch, ny, nx, kind, _ptr(x), _ptr(out), _ptr(ws), nws,
                                   _stream_handle(x)))
    return out


def detrend_inner(x, axis0, naxes, kind):
    """Stand-alone detrend over ``naxes`` (1|2) ADJACENT axes starting at ``axis0`` of a contiguous tensor, whatever follows them
    (xrft.detrend over axes that are not the trailing ones: no transposed copy; xrft/detrend.py:54-55, 64-71, 100-113)."""
    dll = _lib.load()
    if x.dtype not in _DTYPES or not x.is_contiguous():
        raise ValueError("detrend needs a contiguous float/complex tensor")
    batch = int(np.prod(x.shape[:axis0], dtype=np.int64))
    ny = x.shape[axis0] if naxes == 2 else 1
    nx = x.shape[axis0 + naxes - 1]
    inner = int(np.prod(x.shape[axis0 + naxes:], dtype=np.int64))
    if inner > (1 << 30) or nx > (1 << 31) - 1 or ny > (1 << 31) - 1:
        return None  # beyond the extents xrfthip_detrend_inner takes (it would say BAD_ARG): the caller transposes
    nws = int(dll.xrfthip_detrend_inner_workspace_bytes(_DTYPES[x.dtype], batch, inner))
    if nws > max(x.numel() * x.element_size(), 64 << 20):
        return None  # a few samples per element: the partial sums would outgrow the array
    out = torch.empty_like(x)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    _lib.check(dll.xrfthip_detrend_inner(_DTYPES[x.dtype], naxes, batch, ny, nx, inner, kind, _ptr(x), _ptr(out), _ptr(ws), nws, _stream_handle(x)))
    return out


_BLUESTEIN_F64 = [os.environ.get("XRFT_AMD_BLUESTEIN", "float64").lower() not in ("float32", "f32", "fast")]


def bluestein_in_float64(enable=None):
    """float32 data on a transform length too long for Bluestein's algorithm inside one LDS tile (a prime factor above 128 and more than
    ~8800 samples: api._bluestein_1d, three table products around two long plans through global memory) run in float64 between two
    precision changes -- the default: with float32 intermediates stored between the passes, the composition leaves the bins 1e-3 of
    the spectrum's peak 1.3e-3 of relative error, above the 1e-3 every other path holds.  ``bluestein_in_float64(False)`` (or
    XRFT_AMD_BLUESTEIN=float32 in the environment) keeps float32 arithmetic there: the max-norm bound of 1e-3 still holds.
    Bluestein lengths INSIDE a tile (the ERA5 grid's 721 = 7 x 103 latitudes) stay in float32 either way: measured on the GPU they hold
    1.2e-4 per bin (profiles/r04_bluestein_f32.txt).  Returns the setting."""
    if enable is not None:
        _BLUESTEIN_F64[0] = bool(enable)
    return _BLUESTEIN_F64[0]


_WIDER = {torch.float32: torch.float64, torch.complex64: torch.complex128}
_NARROWER = {v: k for k, v in _WIDER.items()}


def convert(x, dtype, out=None):
    """``x`` in the other precision (float32 <-> float64, complex64 <-> complex128) by the library's own kernel (xrfthip_convert); float16 / bfloat16 -> float32, exact:
    the widening behind the calls a half plan declines."""
    dll = _lib.load()
    if x.dtype in _HALF:
        if dtype is not torch.float32:
            raise TypeError(f"convert: {x.dtype} -> {dtype}")
        x = x.contiguous()  # (a view: copied in half precision, 2 bytes per sample)
        if out is None:
            out = torch.empty(x.shape, dtype=dtype, device=x.device)
        elif out.dtype is not dtype or out.numel() != x.numel() or not out.is_contiguous():
            raise ValueError("convert: out does not match")
        _lib.check(dll.xrfthip_convert(_HALF[x.dtype], _lib.F32, x.numel(), _ptr(x), _ptr(out), _stream_handle(x)))
        return out
    if _WIDER.get(x.dtype) is not dtype and _NARROWER.get(x.dtype) is not dtype:
        raise TypeError(f"convert: {x.dtype} -> {dtype}")
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    elif out.dtype is not dtype or out.numel() != x.numel() or not out.is_contiguous():
        raise ValueError("convert: out does not match")
    _lib.check(dll.xrfthip_convert(_DTYPES[x.dtype], _DTYPES[dtype], x.numel(), _ptr(x), _ptr(out), _stream_handle(x)))
    return out


def spectrum_tail(a, b, scale):
    """|a|^2 * scale (real) or a * conj(b) * scale (complex) of transformed fields (xrft.py:740, 825)."""
    dll = _lib.load()
    if not a.is_complex() or not a.is_contiguous() or (b is not None and (b.dtype != a.dtype or b.shape != a.shape or not b.is_contiguous())):
        raise ValueError("spectrum_tail needs contiguous complex tensors of one shape and dtype")
    real_dt = torch.float32 if a.dtype == torch.complex64 else torch.float64
    out = torch.empty(a.shape, dtype=a.dtype if b is not None else real_dt, device=a.device)
    _lib.check(dll.xrfthip_spectrum_tail(_DTYPES[a.dtype], a.numel(), _ptr(a), _ptr(b), _ptr(out), float(scale),
                                         _stream_handle(a)))
    return out


def angle(a):
    """arg(a) in [-pi, pi] of a contiguous complex tensor (numpy.angle; xrft.cross_phase on composed cross spectra)."""
    dll = _lib.load()
    if not a.is_complex():
        raise ValueError("angle needs a complex tensor")
    a = a.contiguous()
    out = torch.empty(a.shape, dtype=torch.float32 if a.dtype == torch.complex64 else torch.float64, device=a.device)
    _lib.check(dll.xrfthip_angle(_DTYPES[a.dtype], a.numel(), _ptr(a), _ptr(out), _stream_handle(a)))
    return out


def coherence(cross, p0, p1):
    """|cross|^2 / (p0 p1) of an averaged cross spectrum (complex) and the two averaged power spectra (real, the matching precision): the magnitude-squared
    coherence where it is composed of three mean spectra.  No clamp; a zero denominator gives what IEEE division gives."""
    dll = _lib.load()
    if not cross.is_complex():
        raise ValueError("coherence needs a complex cross spectrum")
    real_dt = torch.float32 if cross.dtype == torch.complex64 else torch.float64
    if p0.shape != cross.shape or p1.shape != cross.shape or p0.dtype != real_dt or p1.dtype != real_dt or p0.device != cross.device or p1.device != cross.device:
        raise ValueError(f"coherence needs two {real_dt} power spectra of the cross spectrum's shape on its device")
    cross, p0, p1 = cross.contiguous(), p0.contiguous(), p1.contiguous()
    out = torch.empty(cross.shape, dtype=real_dt, device=cross.device)
    _lib.check(dll.xrfthip_coherence(_DTYPES[cross.dtype], cross.numel(), _ptr(cross), _ptr(p0), _ptr(p1), _ptr(out), _stream_handle(cross)))
    return out


def spectrum_tail_axis(a, b, scale, axis, last_is_one):
    """spectrum_tail with the real-dim factor [1, 2, ..., 2, (1)] along ``axis`` (xrft.py:673-682)."""
    dll = _lib.load()
    if not a.is_complex() or not a.is_contiguous() or (b is not None and (b.dtype != a.dtype or b.shape != a.shape or not b.is_contiguous())):
        raise ValueError("spectrum_tail_axis needs contiguous complex tensors of one shape and dtype")
    real_dt = torch.float32 if a.dtype == torch.complex64 else torch.float64
    out = torch.empty(a.shape, dtype=a.dtype if b is not None else real_dt, device=a.device)
    axis = axis % a.dim()
    outer = int(np.prod(a.shape[:axis], dtype=np.int64))
    inner = int(np.prod(a.shape[axis + 1:], dtype=np.int64))
    _lib.check(dll.xrfthip_spectrum_tail_axis(_DTYPES[a.dtype], outer, a.shape[axis], inner, int(bool(last_is_one)), _ptr(a), _ptr(b),
                                              _ptr(out), float(scale), _stream_handle(a)))
    return out


def gather_axis(x, axis, index=None, roll=0):
    """``x`` re-ordered along ``axis``: out[..., i, ...] = x[..., index[i], ...] (``index``: host int array) or numpy.roll by
    ``roll``.  A device copy kernel (xrfthip_gather_axis): no torch arithmetic."""
    dll = _lib.load()
    if not x.is_contiguous():
        x = x.contiguous()
    axis = axis % x.dim()
    n_in = x.shape[axis]
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    idx = None
    n_out = n_in
    if index is not None:
        idx = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).to(x.device)
        n_out = idx.numel()
    shape = list(x.shape)
    shape[axis] = n_out
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _lib.check(dll.xrfthip_gather_axis(x.element_size(), outer, n_out, inner, n_in, _ptr(idx), int(roll), _ptr(x), _ptr(out),
                                       _stream_handle(x)))
    return out


def table_mul(x, table, n_out):
    """out[..., j] = (j < n ? x[..., j] : 0) * table[j], j < n_out, complex result: zero padding / truncation with a pointwise factor
    (the pointwise steps of Bluestein's algorithm through global memory)."""
    dll = _lib.load()
    x = x.contiguous()
    n_in = x.shape[-1]
    batch = x.numel() // max(n_in, 1)
    cdt = torch.complex64 if x.dtype in (torch.float32, torch.complex64) else torch.complex128
    if table.dtype != cdt or table.numel() < min(n_in, n_out) or not table.is_contiguous():
        raise ValueError("table_mul needs a contiguous complex table of the data's precision with min(n, n_out) entries")
    out = torch.empty(list(x.shape[:-1]) + [n_out], dtype=cdt, device=x.device)
    _lib.check(dll.xrfthip_table_mul(_DTYPES[x.dtype], batch, n_in, n_out, _ptr(x), _ptr(table), _ptr(out), _stream_handle(x)))
    return out


def device_type():
    """torch device type the bound library computes on ('cuda'; 'cpu' only for the emulated test build)."""
    return _lib.device()


def reduce_axis(x, axis, scale=1.0):
    """scale * sum of ``x`` over ``axis`` (a device kernel, float64 accumulation in index order: bit-reproducible); the mean over a
    batch dimension with scale = 1 / n (the reference's users average isotropic spectra over the batch, test_xrft.py:1011-1013)."""
    dll = _lib.load()
    if x.dtype not in _DTYPES:
        raise TypeError(f"reduce_axis: unsupported dtype {x.dtype}")
    x = x.contiguous()
    axis = axis % x.dim()
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    out = torch.empty(list(x.shape[:axis]) + list(x.shape[axis + 1:]), dtype=x.dtype, device=x.device)
    _lib.check(dll.xrfthip_reduce_axis(_DTYPES[x.dtype], outer, x.shape[axis], inner, _ptr(x), _ptr(out), float(scale), _stream_handle(x)))
    return out


def isotropize(x, binmap_dev, nbins):
    """Radial bin-sum of the last two axes of ``x`` with a device int32 bin map (xrft/xrft.py:993-1004)."""
    dll = _lib.load()
    ny, nx = x.shape[-2], x.shape[-1]
    batch = x.numel() // max(ny * nx, 1)
    cplx = x.is_complex()
    iso = torch.empty((batch, nbins), dtype=torch.complex128 if cplx else torch.float64, device=x.device)
    nws = int(dll.xrfthip_isotropize_workspace_bytes(_DTYPES[x.dtype], batch, ny, nx, nbins))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)  # per-workgroup partial sums (added in a fixed order: bit-reproducible)
    _lib.check(dll.xrfthip_isotropize(_DTYPES[x.dtype], batch, ny, nx, _ptr(x), _ptr(binmap_dev), nbins, _ptr(iso), _ptr(ws), nws,
                                      _stream_handle(x)))
    return iso
