"""Host side of the HiFT vocoder: mirrors `CausalHiFTGenerator.inference`
(CosyVoice/cosyvoice/hifigan/generator.py:713-726) over the C ABI.

torch is used for device memory and streams only; all arithmetic happens in
libfy_cosy3's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from ._lib import FY_DIRECT, FY_INCREMENTAL, FY_NO_FINALIZE, FY_PRECISE, check  # noqa: F401
from .spec import HiftCfg


def _cfg_struct(cfg: HiftCfg) -> _lib.HiftConfig:
    c = _lib.HiftConfig()
    _lib.lib().fy_hift_default_config(C.byref(c))
    c.mel, c.base, c.harmonics, c.sampling_rate = cfg.mel, cfg.base, cfg.harmonics, 24000
    c.nsf_alpha, c.nsf_sigma, c.voiced_thr = cfg.nsf_alpha, cfg.nsf_sigma, cfg.voiced_thr
    for i in range(3):
        c.ups[i], c.up_k[i], c.rb_k[i], c.rb_d[i], c.src_rb_k[i] = cfg.ups[i], cfg.up_k[i], cfg.rb_k[i], cfg.rb_d[i], cfg.src_rb_k[i]
    c.n_fft, c.hop, c.lrelu, c.audio_limit = cfg.n_fft, cfg.hop, cfg.lrelu, cfg.audio_limit
    c.pre_look_right, c.f0_ch = cfg.pre_look_right, cfg.f0_ch
    return c


def stream_new_samples(frames: int, finalize: bool, delivered: int, up: int = 480) -> int:
    """Samples an incremental call brings: a chunk holds 8 frames back (3 + 4 of look-ahead and one of samples,
    generator.py:713-726), the final call nothing; `delivered` are the stream's samples so far (0 on its first call)."""
    return up * (frames if finalize else frames - 8) - delivered


class HiftEngine:
    """Batched, ragged HiFT vocoder on one GPU.

    weights: the hift.pt state_dict (reference key names, fp32 CUDA tensors)."""

    def __init__(self, weights: Dict[str, torch.Tensor], cfg: HiftCfg = HiftCfg(), max_batch: int = 8,
                 max_frames: int = 1500, device: Optional[torch.device] = None):
        self.cfg = cfg
        self.device = device or next(iter(weights.values())).device
        self.max_batch, self.max_frames = max_batch, max_frames
        self._h = C.c_void_p()
        arr, keep = _lib.tensor_table(weights)
        cs = _cfg_struct(cfg)
        with torch.cuda.device(self.device):
            check(_lib.lib().fy_hift_create(C.byref(self._h), C.byref(cs), arr, len(weights), max_batch, max_frames,
                                            self._stream()))
        del keep

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if self._h:
            _lib.lib().fy_hift_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prep(self, mel: torch.Tensor, frames: Optional[Sequence[int]]):
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.dim() == 3 and mel.shape[1] == self.cfg.mel
        mel = mel.contiguous()
        B, _, Fmax = mel.shape
        frames = [Fmax] * B if frames is None else list(frames)
        return mel, B, Fmax, _lib.int_array(frames)

    def inference(self, speech_feat: torch.Tensor, rand_ini: torch.Tensor, sine_noise: torch.Tensor,
                  frames: Optional[Sequence[int]] = None, flags: int = 0, want_source: bool = False, finalize: bool = True,
                  incremental: bool = False):
        """speech_feat (B, 80, Fmax) -> (wav (B, 480*Fmax), source (B, 1, 480*Fmax) or None).
        Samples past 480*frames[b] of a shorter utterance are left untouched (zeros).
        finalize=False (generator.py:713-726, a streaming chunk): 3 + 4 frames are look-ahead and one frame of samples is held
        back: utterance b is valid in wav[b, :480*(frames[b] - 8)], its source in [:480*(frames[b] - 3)].
        incremental (one utterance, the whole mel so far): this call continues the handle's stream - only the samples beyond those
        the stream has delivered are computed and written, wav[:, stream_samples() before the call : the end above]; the rest
        stays zero.  Same values as without the flag.  A finalize call ends the stream; `stream_reset` starts a new one."""
        if not finalize:
            flags |= FY_NO_FINALIZE
        if incremental:
            flags |= FY_INCREMENTAL                     # (with want_source the library refuses: there is no whole source)
        mel, B, Fmax, fr = self._prep(speech_feat, frames)
        S = Fmax * self.cfg.upsample_total
        assert sine_noise.is_cuda and sine_noise.is_contiguous() and sine_noise.shape[-2] >= S
        wav = torch.zeros(B, S, device=mel.device, dtype=torch.float32)
        src = torch.zeros(B, S, device=mel.device, dtype=torch.float32) if want_source else None
        check(_lib.lib().fy_hift_infer(self._h, mel.data_ptr(), fr, B, Fmax, rand_ini.data_ptr(), sine_noise.data_ptr(),
                                       wav.data_ptr(), src.data_ptr() if want_source else None, flags, self._stream()))
        return wav, (src[:, None] if want_source else None)

    def stream_reset(self):
        """Forget the incremental stream: the next incremental call starts a new one."""
        check(_lib.lib().fy_hift_stream_reset(self._h))

    def stream_samples(self) -> int:
        """Samples the incremental calls of the current stream have delivered (0: the next call computes everything)."""
        return int(_lib.lib().fy_hift_stream_samples(self._h))

    def stream_window(self) -> int:
        """Mel frames the last incremental call ran through the network."""
        return int(_lib.lib().fy_hift_stream_window(self._h))

    # ---- stream slots: several streams through one incremental pass (csrc/hift.hip: fy_hift_infer_streams)
    def open_streams(self, n_slots: int, store_frames: Optional[int] = None):
        """Give the handle `n_slots` (<= max_batch) incremental streams; the work buffers stay the handle's own.
        store_frames: also a mel store of that many frames per slot (n_slots x 80 x store_frames fp32, fy_hift_streams_store):
        `stream_slot_push` appends a flow call's rows to it on the device and `inference_streams(..., mels=None)` reads it.  When
        the device lacks the memory this raises FyError with the byte count and the session stays open without a store."""
        with torch.cuda.device(self.device):
            check(_lib.lib().fy_hift_streams_open(self._h, n_slots))
            if store_frames is not None:
                check(_lib.lib().fy_hift_streams_store(self._h, int(store_frames)))

    def close_streams(self):
        check(_lib.lib().fy_hift_streams_close(self._h))

    def streams_bytes(self) -> int:
        """Device bytes of the open session (0: none)."""
        return int(_lib.lib().fy_hift_streams_bytes(self._h))

    def stream_slot_reset(self, slot: int):
        check(_lib.lib().fy_hift_stream_slot_reset(self._h, slot))

    def stream_slot_samples(self, slot: int) -> int:
        """Samples the slot's stream has delivered (0: its next call computes everything; -1: no such slot)."""
        return int(_lib.lib().fy_hift_stream_slot_samples(self._h, slot))

    def stream_slot_window(self, slot: int) -> int:
        """Mel frames of the slot's stream the last call ran through the network (-1: no such slot)."""
        return int(_lib.lib().fy_hift_stream_slot_window(self._h, slot))

    def stream_slot_push(self, slots: Sequence[int], mel: torch.Tensor, first: Sequence[int], count: Sequence[int]):
        """ONE copy kernel: row i of `mel` (n, 80, F) - a flow call's output - frames [first[i], first[i] + count[i]) go behind
        what slot slots[i]'s store holds.  Nothing passes through the host; the slots' counts advance."""
        n = len(slots)
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.dim() == 3 and mel.shape[0] == n and mel.shape[1] == self.cfg.mel
        assert mel.is_contiguous() and len(first) == n and len(count) == n
        check(_lib.lib().fy_hift_stream_slot_push(self._h, _lib.int_array(list(slots)), n, mel.data_ptr(), mel.shape[2], _lib.int_array(first),
                                                  _lib.int_array(count), self._stream()))

    def stream_slot_frames(self, slot: int) -> int:
        """Mel frames the slot's store holds (-1: no such slot)."""
        return int(_lib.lib().fy_hift_stream_slot_frames(self._h, slot))

    def inference_streams(self, slots: Sequence[int], mels: Optional[Sequence[torch.Tensor]], rand_ini: torch.Tensor, sine_noise: torch.Tensor,
                          finalize: Sequence[bool], flags: int = 0, frames: Optional[Sequence[int]] = None):
        """Continue the streams of `slots` in one pass.  mels[i]: (1, 80, F_i) or (80, F_i), stream i's whole mel so far (separate
        tensors of any lengths); finalize[i]: stream i's last call.  Returns a list of 1-D tensors, stream i's NEW samples
        [stream_slot_samples(slots[i]) before the call, 480 (F_i - 8) or 480 F_i) - views of one (n, wav_ld) buffer - the same
        values `inference(..., incremental=True)` writes there for that stream alone.
        mels=None: every stream's mel is what its slot's store holds (`stream_slot_push`) - all of it, or its first frames[i]
        frames: the same samples, bit for bit, as the call given those frames as tensors."""
        n = len(slots)
        assert n >= 1 and len(finalize) == n
        if mels is None:
            frames = [self.stream_slot_frames(s) for s in slots] if frames is None else [int(f) for f in frames]
            ptrs = (C.c_void_p * n)()
        else:
            assert len(mels) == n
            ms = []
            for m in mels:
                m = m[0] if m.dim() == 3 else m
                assert m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.shape[0] == self.cfg.mel
                ms.append(m.contiguous())
            frames = [int(m.shape[1]) for m in ms]
            ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in ms])
        up = self.cfg.upsample_total
        assert sine_noise.is_cuda and sine_noise.is_contiguous() and sine_noise.shape[-2] >= up * max(frames)
        # what each slot has delivered; a slot given fewer frames than its last call (samples / up + 8) starts over, as in the library
        done = [max(self.stream_slot_samples(s), 0) for s in slots]
        done = [d if F >= d // up + 8 else 0 for d, F in zip(done, frames)]
        wav_ld = max(1, max(stream_new_samples(F, bool(fin), d, up) for F, fin, d in zip(frames, finalize, done)))
        wav = torch.zeros(n, wav_ld, device=self.device, dtype=torch.float32)
        n_new = (C.c_int32 * n)()
        check(_lib.lib().fy_hift_infer_streams(self._h, _lib.int_array(list(slots)), n, ptrs, _lib.int_array(frames), _lib.int_array(frames),
                                               _lib.int_array([int(bool(f)) for f in finalize]), rand_ini.data_ptr(), sine_noise.data_ptr(),
                                               wav.data_ptr(), wav_ld, n_new, flags, self._stream()))
        return [wav[i, : n_new[i]] for i in range(n)]

    def f0(self, speech_feat, frames=None):
        mel, B, Fmax, fr = self._prep(speech_feat, frames)
        out = torch.zeros(B, Fmax, device=mel.device, dtype=torch.float32)
        check(_lib.lib().fy_hift_f0(self._h, mel.data_ptr(), fr, B, Fmax, out.data_ptr(), self._stream()))
        return out

    def source(self, f0, rand_ini, sine_noise, frames=None):
        B, Fmax = f0.shape
        fr = _lib.int_array([Fmax] * B if frames is None else list(frames))
        out = torch.zeros(B, Fmax * self.cfg.upsample_total, device=f0.device, dtype=torch.float32)
        check(_lib.lib().fy_hift_source(self._h, f0.contiguous().data_ptr(), fr, B, Fmax, rand_ini.data_ptr(),
                                        sine_noise.data_ptr(), out.data_ptr(), self._stream()))
        return out[:, None]

    def decode(self, speech_feat, source, frames=None, flags: int = 0):
        mel, B, Fmax, fr = self._prep(speech_feat, frames)
        S = Fmax * self.cfg.upsample_total
        src = source.reshape(B, S).contiguous()
        wav = torch.zeros(B, S, device=mel.device, dtype=torch.float32)
        check(_lib.lib().fy_hift_decode(self._h, mel.data_ptr(), src.data_ptr(), fr, B, Fmax, wav.data_ptr(), flags,
                                        self._stream()))
        return wav

    def tap(self, name: str, B: int, Fmax: int) -> torch.Tensor:
        """Internal tensor of the last call in the reference's (B, C, L) layout."""
        rows, cols = C.c_int64(), C.c_int64()
        cap = B * (Fmax * self.cfg.upsample_total + 1) * 64
        buf = torch.empty(cap, device=self.device)
        check(_lib.lib().fy_hift_tap(self._h, name.encode(), buf.data_ptr(), C.byref(rows), C.byref(cols), self._stream()))
        return buf[: B * rows.value * cols.value].view(B, rows.value, cols.value).transpose(1, 2).contiguous()

    def resblock(self, index: int, x: torch.Tensor, flags: int = 0) -> torch.Tensor:
        """One main-stack ResBlock on x (B, C, L) (reference layout) -> (B, C, L)."""
        xcl = x.transpose(1, 2).contiguous()
        y = torch.empty_like(xcl)
        B, L, _ = xcl.shape
        check(_lib.lib().fy_hift_resblock(self._h, index, xcl.data_ptr(), y.data_ptr(), B, L, flags, self._stream()))
        return y.transpose(1, 2).contiguous()
