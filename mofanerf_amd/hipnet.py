"""Device-side state of one ``NeRF`` for the HIP path: packed weights, folded biases, workspace.

``HipNet`` never computes anything itself — it owns the buffers the C ABI needs (allocated through
PyTorch's caching allocator on the current HIP device) and issues the ``mofa_net_*`` calls on the
current stream.
"""
from __future__ import annotations

import threading
import weakref
from typing import Optional

import torch

from . import lib
from .model import NeRF


def unwrap(net):
    """Callers may hand the nets wrapped in ``nn.DataParallel`` (run_fit.py:166-167)."""
    return net.module if isinstance(net, torch.nn.DataParallel) else net


def _freqs_of(ch: int, what: str) -> int:
    """Encoding width -> number of frequencies: 3 + 6 L (get_embedder, models/model.py:48-63; L = 0 is i_embed = -1)."""
    if ch < 3 or (ch - 3) % 6:
        raise lib.MofaError(f"{what} = {ch} is not a positional-encoding width 3 + 6*L (models/model.py:48-63)")
    return (ch - 3) // 6


class HipNet:
    def __init__(self, net: NeRF, point_freqs: int = 10, weak: bool = False, embedded: bool = False):
        """``point_freqs``: ``multires`` of the point encoding the renderer feeds this network (tools/config_parser.py:53).  The module
        alone only knows ``input_ch = (3 + 6*multires) + input_ch_expCodes`` (tools/create_model_condition.py:25), so the split between
        per-point encoding columns and per-call expression-code columns comes from the renderer's ``embed_fn``; every other width is
        read off the module.  The resulting ``MofaNetShape`` is then checked against EVERY ``Linear`` of the module
        (``mofa_net_layer_dims``) — a module the plan does not describe is refused here, never mis-read by a kernel.

        ``weak``: keep only a weak reference to the module (the Linear children are still held) — for caches keyed weakly on the
        module itself (model._EMBEDDED_CACHE): a strong back-reference from the value would keep the key alive for ever.

        ``embedded``: the state behind ``NeRF.forward`` on ALREADY-EMBEDDED per-point inputs (``forward_embedded``) only.  There every
        input column is a per-point column, so neither the encoding / expression split nor ``input_ch_views = 3 + 6 L`` means
        anything: like the reference's module (models/model.py:85-137) any ``input_ch`` / ``input_ch_views`` is accepted, the Linear
        shapes are checked against the constructor's own rule, and the folded entry points (which need the C plan) are unavailable."""
        if not isinstance(net, NeRF):
            raise lib.MofaError(f"expected mofanerf_amd.model.NeRF, got {type(net).__name__}")
        self._net_strong = None if weak else net
        self._net_weak = weakref.ref(net)
        self.D, self.W = int(net.D), int(net.W)
        self.embedded = bool(embedded)
        self._L = lib.load()
        self._linears = net.ordered_linears()
        self.ch_shape, self.ch_tex = int(net.input_ch_shapeCodes), int(net.input_ch_textureCodes)
        if self.embedded:
            D, W = self.D, self.W
            self.point_freqs, self.view_freqs, self.shape = 0, None, None
            self.ch_pe, self.ch_exp, self.ch_views = int(net.input_ch), 0, int(net.input_ch_views)
            want = ([(W, self.ch_pe)] + [(W, W)] * 3 +
                    [(W, self.ch_shape + W)] + [(W, W)] * 4 + [(W, self.ch_shape + 2 * W)] + [(W, W)] * (D - 6) +
                    [(W, self.ch_tex + W)] + [(W, W)] * 4 + [(W, self.ch_tex + 2 * W)] + [(W, W)] * (D - 6) +
                    [(W // 2, self.ch_views + W), (1, W), (3, W // 2)])
            got = [(l.out_features, l.in_features) for l in self._linears]
            if D < 6 or got != want:
                bad = next((i for i, (g, w_) in enumerate(zip(got, want)) if g != w_), min(len(got), len(want)))
                raise lib.MofaError(f"layer {bad} of the module is not what NeRF(D={D}, W={W}, input_ch={self.ch_pe}, input_ch_views={self.ch_views}, "
                                    f"input_ch_shapeCodes={self.ch_shape}, input_ch_textureCodes={self.ch_tex}) builds (models/model.py:85-118); "
                                    "refusing to pack it")
        else:
            self._init_plan(net, point_freqs)
        # launch verdicts (include/mofanerf_hip.h, MOFA_VERDICT_WORDS): sticky words on the device that the verification kernel behind
        # every chained launch raises, an asynchronous pinned mirror, and the event that says the mirror is current.  The mirror is
        # written by copies enqueued on ONE stream at a time (the stream the caller runs on; side streams of the multi-stream
        # inference path do not snapshot — the renderer does, on the main stream after it has joined them), and the state is
        # guarded by a lock: the PNG sink's workers look at per-frame tokens (verdict_token) of their own, never at this mirror.
        self._verdict: Optional[torch.Tensor] = None
        self._verdict_host: Optional[torch.Tensor] = None
        self._verdict_event: Optional[torch.cuda.Event] = None
        self._verdict_lock = threading.Lock()
        if torch.cuda.is_available() and next(net.parameters()).is_cuda:
            lib.device_init(next(net.parameters()).device)       # census + self-check (the library's one synchronising call) — here, not in a forward
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._folded: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._packed_t: Optional[torch.Tensor] = None
        self._packed_t_key = None
        self._bws: Optional[torch.Tensor] = None
        self._nominal, self._nominal_key = None, None
        self.gate_stats_dev: Optional[torch.Tensor] = None   # [2] int64 on the device: samples / live samples of the gated calls
        self.last_gated: Optional[int] = None                 # route of the last gated call: 1 = gated, 0 = the full forward ran

    @property
    def net(self) -> Optional[NeRF]:
        return self._net_strong if self._net_strong is not None else self._net_weak()

    def _init_plan(self, net: NeRF, point_freqs: int) -> None:
        self.point_freqs = int(point_freqs)
        self.ch_pe = 3 + 6 * self.point_freqs
        self.ch_exp = int(net.input_ch) - self.ch_pe
        if self.ch_exp < 0:
            raise lib.MofaError(f"NeRF.input_ch = {net.input_ch} is narrower than the point encoding it is fed (multires = {point_freqs} "
                                f"-> {self.ch_pe} columns); input_ch = (3 + 6*multires) + input_ch_expCodes (tools/create_model_condition.py:25)")
        self.view_freqs = _freqs_of(int(net.input_ch_views), "NeRF.input_ch_views")
        self.ch_views = 3 + 6 * self.view_freqs
        self.shape = lib.NetShape(net.D, net.W, self.point_freqs, self.view_freqs, self.ch_exp, self.ch_shape, self.ch_tex)
        n_plan = self._L.mofa_net_num_layers(self.shape)
        if n_plan < 0:
            raise lib.MofaError(f"unsupported network shape {self.shape}: {self._L.mofa_last_error().decode()}")
        if n_plan != len(self._linears):
            raise lib.MofaError(f"layer count mismatch: the module has {len(self._linears)} Linear layers, the plan of {self.shape} has {n_plan}")
        import ctypes as C
        no, ni = C.c_int32(), C.c_int32()
        for li, l in enumerate(self._linears):
            lib.check(self._L.mofa_net_layer_dims(self.shape, li, C.byref(no), C.byref(ni)), "mofa_net_layer_dims")
            if (l.out_features, l.in_features) != (no.value, ni.value):
                raise lib.MofaError(f"layer {li} of the module is Linear({l.in_features} -> {l.out_features}) but {self.shape} has "
                                    f"Linear({ni.value} -> {no.value}) there: the module was not built by NeRF(D, W, input_ch, ...) with "
                                    "these widths (tools/create_model_condition.py:16-34); refusing to pack it")

    def _need_plan(self, what: str) -> None:
        if self.shape is None:
            raise lib.MofaError(f"{what}: this HipNet was built for NeRF.forward on embedded inputs only (embedded=True); the folded "
                                "renderer path needs HipNet(net, point_freqs=multires)")

    # -- launch verdicts ----------------------------------------------------------------------------
    def verdict_ptr(self, device) -> int:
        """Device pointer of this network's sticky verdict words (created zeroed on first use)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:       # "cuda" = the current device: compare like with like
            device = torch.device("cuda", torch.cuda.current_device())
        if self._verdict is None or self._verdict.device != device:
            # a network built on the CPU and moved with .cuda() afterwards meets its device HERE for the first time: take the per-device
            # initialisation now (cached per device and process: later calls cost a dictionary look-up), or the wide networks would
            # stay on the per-layer launches for the life of the process
            lib.device_init(device)
            with self._verdict_lock:
                self._verdict = torch.zeros(lib.VERDICT_WORDS, dtype=torch.int32, device=device)
                self._verdict_host = torch.zeros(lib.VERDICT_WORDS, dtype=torch.int32).pin_memory()
                self._verdict_event = None
        return self._verdict.data_ptr()

    def snapshot_verdict(self) -> None:
        """Enqueue a copy of the verdict words into the pinned mirror behind the launches issued so far ON THE CURRENT STREAM (no host
        synchronisation)."""
        if self._verdict is None:
            return
        with self._verdict_lock:
            self._verdict_host.copy_(self._verdict, non_blocking=True)
            if self._verdict_event is None:
                self._verdict_event = torch.cuda.Event()
            self._verdict_event.record()

    def _raise_incomplete(self, w) -> None:
        raise lib.MofaError(f"a chained launch (k_net_chain) of {self.shape} did not complete: "
                            f"{'a dependency wait timed out; ' if w[0] & 1 else ''}{'tiles missing; ' if w[0] & 2 else ''}"
                            f"last launch finished {w[3]} of {w[4]} tiles, {w[5]} bad of {w[1]} chained launches — its outputs were "
                            "overwritten with NaN.  (A CU-masked stream or a changed compute partition leaves XCD queues unworked; several "
                            "PROCESSES sharing this device can starve a dependency wait — the chained launch assumes one process per GPU; "
                            "MOFA_CHAIN=0 selects the per-layer launches: the same bits, about 1 % slower.)")

    def check_verdict(self, block: bool = False) -> None:
        """Raise ``MofaError`` if a chained launch of this network ended incomplete (its outputs were overwritten with NaN by the
        verification kernel).  ``block=False`` looks only if the last snapshot has already arrived — the form the launch paths use before
        every call, so a failure surfaces at the next call at the latest without ever stalling the host; ``block=True`` waits for it
        (end of a frame's consumer: bench, tests, ``render_path``).  Call it from the thread that issues the launches: on a failure it
        re-arms the sticky device words (an enqueue on the current stream)."""
        with self._verdict_lock:
            ev = self._verdict_event
            if ev is None:
                return
            if block:
                ev.synchronize()
            elif not ev.query():
                return
            w = self._verdict_host.tolist()
            if w[0] == 0:
                return
            self._verdict.zero_()
            self._verdict_event = None
        self._raise_incomplete(w)

    def verdict_token(self):
        """A per-FRAME look at the verdict words, for a consumer on another thread (the PNG sink's workers): the words are copied into a
        pinned buffer of the token's own behind everything issued on the current stream so far, with an event of its own.  ``token()``
        waits for THAT copy and raises ``MofaError`` if a chained launch before it ended incomplete — pure host work on state nobody
        else touches (the shared mirror above belongs to the launching thread).  Returns ``None`` when this network never launched."""
        if self._verdict is None:
            return None
        host = torch.empty(lib.VERDICT_WORDS, dtype=torch.int32).pin_memory()
        host.copy_(self._verdict, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()

        def look():
            ev.synchronize()
            w = host.tolist()
            if w[0] != 0:
                self._raise_incomplete(w)
        return look

    def chained_launches(self, block: bool = True) -> int:
        """Number of chained launches verified so far (tests: was the chained form really taken?)."""
        self.snapshot_verdict()
        with self._verdict_lock:
            if self._verdict_event is None:
                return 0
            self._verdict_event.synchronize()
            return int(self._verdict_host[1])

    def invalidate(self):
        """Forget the packed / transposed copies of the weights (they are rebuilt on the next call).  Needed only
        after an edit made through ``.data``, which bypasses the version counter the cache keys on."""
        self._packed_key = self._packed_t_key = self._nominal_key = None

    # -- weights -----------------------------------------------------------------------------------
    def _weights(self):
        ws = [l.weight.detach() for l in self._linears]
        bs = [l.bias.detach() for l in self._linears]
        for t in ws + bs:
            if not t.is_cuda:
                raise lib.MofaError("network parameters must live on the GPU (net.cuda()); there is no CPU path")
        return [w.contiguous() for w in ws], [b.contiguous() for b in bs]

    def _key(self):
        return tuple((l.weight.data_ptr(), l.weight._version) for l in self._linears)

    def packed(self) -> torch.Tensor:
        """Panel-packed weights; re-packed only when a parameter changed (optimizer step / load_state_dict)."""
        self._need_plan("packed()")
        key = self._key()
        if self._packed is None or key != self._packed_key:
            ws, _ = self._weights()
            n = self._L.mofa_net_packed_floats(self.shape)
            if self._packed is None or self._packed.numel() != n or self._packed.device != ws[0].device:
                self._packed = torch.empty(n, dtype=torch.float32, device=ws[0].device)
            lib.check(self._L.mofa_net_pack(self.shape, lib.ptr_array(ws), lib.ptr(self._packed), lib.stream()),
                      "mofa_net_pack")
            self._packed_key = key
        return self._packed

    def packed_t(self) -> torch.Tensor:
        """Transposed weight panels for the backward-data GEMMs (re-packed when a parameter changed)."""
        key = self._key()
        if self._packed_t is None or key != self._packed_t_key:
            ws, _ = self._weights()
            n = self._L.mofa_net_packed_t_floats(self.shape)
            if self._packed_t is None or self._packed_t.numel() != n or self._packed_t.device != ws[0].device:
                self._packed_t = torch.empty(n, dtype=torch.float32, device=ws[0].device)
            lib.check(self._L.mofa_net_pack_t(self.shape, lib.ptr_array(ws), lib.ptr(self._packed_t), lib.stream()),
                      "mofa_net_pack_t")
            self._packed_t_key = key
        return self._packed_t

    def backward_workspace(self, n_points: int, device, with_weight_grads: bool = False) -> torch.Tensor:
        n = self._L.mofa_net_backward_workspace_floats(self.shape, n_points, int(bool(with_weight_grads)))
        if self._bws is None or self._bws.numel() < n or self._bws.device != device:
            self._bws = torch.empty(n, dtype=torch.float32, device=device)
        return self._bws

    def fold(self, exp_code: torch.Tensor, shape_code: torch.Tensor, tex_code: torch.Tensor) -> torch.Tensor:
        """Per-call folded biases from the (already modulated) expression code [ch_exp], shape code [ch_shape] and
        texture code [ch_tex]."""
        self._need_plan("fold()")
        ws, bs = self._weights()
        n = self._L.mofa_net_folded_floats(self.shape)
        if self._folded is None or self._folded.device != ws[0].device:
            self._folded = torch.empty(n, dtype=torch.float32, device=ws[0].device)
        e = exp_code.detach().reshape(-1).float().contiguous()
        s = shape_code.detach().reshape(-1).float().contiguous()
        t = tex_code.detach().reshape(-1).float().contiguous()
        self.check_codes(e, s, t)
        lib.check(self._L.mofa_net_fold(self.shape, lib.ptr_array(ws), lib.ptr_array(bs), lib.ptr(e), lib.ptr(s),
                                        lib.ptr(t), lib.ptr(self._folded), lib.stream()), "mofa_net_fold")
        return self._folded

    def check_codes(self, e, s, t) -> None:
        """The widths the networks were BUILT for (the reference fails inside the first Linear on a mismatch, model.py:129-133)."""
        got, want = (e.numel(), s.numel(), t.numel()), (self.ch_exp, self.ch_shape, self.ch_tex)
        if got != want:
            raise lib.MofaError(f"expression / shape / texture code widths {got} do not match the network's {want} "
                                f"(input_ch - (3 + 6*multires), input_ch_shapeCodes, input_ch_textureCodes of {self.shape})")

    def workspace(self, n_points: int, n_rays: int, device, slot: int = 0, floats: Optional[int] = None) -> torch.Tensor:
        """Activation buffers of one sub-batch.  ``slot`` > 0: an independent buffer for a sub-batch that runs concurrently on
        another stream."""
        n = self._L.mofa_net_workspace_floats(self.shape, n_points, n_rays) if floats is None else int(floats)
        if self._ws is None:
            self._ws = {}
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < n or ws.device != device:
            ws = self._ws[slot] = torch.empty(n, dtype=torch.float32, device=device)
        return ws

    def gate_stats_buffer(self, device) -> torch.Tensor:
        """The device-side counters of the gated calls, created zeroed on first use — on the CALLER's stream: whoever forks side streams
        calls this first, so that no side stream zero-fills what another already adds to."""
        if self.gate_stats_dev is None or self.gate_stats_dev.device != device:
            self.gate_stats_dev = torch.zeros(2, dtype=torch.int64, device=device)
        return self.gate_stats_dev

    def _forward_gated(self, rays_o, rays_d, z, z_row_stride, pts, viewdirs, R, S, raw_out, folded, slot, snapshot):
        import ctypes as C
        view = self._linears[-3]
        dev = viewdirs.device
        # the SAME per-slot buffer as the full forward's, grown only when this call can gate (the library sizes it by the route it will take)
        with torch.cuda.device(dev):
            ws = self.workspace(R * S, R, dev, slot, floats=self._L.mofa_net_forward_gated_workspace_floats(self.shape, R * S, R))
        stats = self.gate_stats_buffer(dev)
        route = C.c_int32(0)
        self.check_verdict()
        lib.check(self._L.mofa_net_forward_gated(self.shape, lib.ptr(self.packed()),
                                                 lib.ptr(folded if folded is not None else self._folded),
                                                 lib.ptr(view.weight.detach().contiguous()), lib.ptr(view.bias.detach().contiguous()),
                                                 lib.ptr(rays_o), lib.ptr(rays_d), lib.ptr(z), z_row_stride, lib.ptr(pts),
                                                 lib.ptr(viewdirs), R, S, lib.ptr(ws), lib.ptr(raw_out), None,
                                                 stats.data_ptr(), C.byref(route), self.verdict_ptr(dev), lib.stream()),
                  "mofa_net_forward_gated")
        self.last_gated = int(route.value)
        if snapshot:
            self.snapshot_verdict()
        return raw_out

    # -- NeRF.forward on ALREADY-EMBEDDED per-point inputs (the reference module's own call form) ---------------
    def _nominal_pack(self):
        """Weights packed WITHOUT folding: every input column is a per-point column, in the reference's concat order
        ([pts93], [bm50 | xyz], [bm50 | xyz | h], [tex256 | sigma], [tex256 | sigma | h], [views27 | rgbCodes])."""
        # the nominal pack also caches bias COPIES (padded), so its key covers the biases too — a bias-only update (a bias-only
        # optimizer, bias.copy_(...)) must not be served stale rows; the folded path re-reads biases on every call
        key = self._key() + tuple((l.bias.data_ptr(), l.bias._version) for l in self._linears)
        if getattr(self, "_nominal", None) is not None and self._nominal_key == key:
            return self._nominal
        L, st = self._L, lib.stream()
        D, W = self.D, self.W
        Wp, Hp = (W + 63) // 64 * 64, (W // 2 + 63) // 64 * 64
        ws, bs = self._weights()
        dev = ws[0].device
        bim0, bim_skip, uv0, uv_skip, view = 4, 9, 4 + D, 9 + D, 4 + 2 * D
        cond = {bim0: self.ch_shape, bim_skip: self.ch_shape, uv0: self.ch_tex, uv_skip: self.ch_tex}
        r16 = lambda v: (v + 15) // 16 * 16
        packed, biases = [], []
        for li, (w, b) in enumerate(zip(ws, bs)):
            n_out, ld = w.shape
            if li >= view + 1:                                   # heads: dense rows [n_out, k_padded]
                kp = Wp if li == view + 1 else Hp
                dense = torch.zeros(n_out, kp, dtype=torch.float32, device=dev)
                dense[:, :ld] = w
                packed.append(dense)
                biases.append(b.clone())
                continue
            Np = Hp if li == view else Wp
            if li == 0:
                parts = [(0, ld, r16(ld))]
            elif li in cond:
                c, cpad = cond[li], r16(cond[li])
                parts = ([(0, c, cpad)] if c else []) + [(c, W, Wp)] + ([(c + W, W, Wp)] if li in (bim_skip, uv_skip) else [])
            elif li == view:
                parts = [(0, self.ch_views, r16(self.ch_views)), (self.ch_views, W, Wp)]
            else:
                parts = [(0, ld, Wp)]
            buf = torch.zeros(Np * sum(p[2] for p in parts), dtype=torch.float32, device=dev)
            panel0 = 0
            for col0, ncols, kpad in parts:
                lib.check(L.mofa_pack_panels(lib.ptr(w), n_out, ld, col0, ncols, lib.ptr(buf), Np, panel0, kpad, st), "mofa_pack_panels")
                panel0 += kpad // 16
            bp = torch.zeros(Np, dtype=torch.float32, device=dev)
            bp[:n_out] = b
            packed.append(buf)
            biases.append(bp)
        self._nominal, self._nominal_key = (packed, biases), key
        return self._nominal

    def forward_embedded(self, pts93, bm50, views27, tex256) -> torch.Tensor:
        """``NeRF.forward(input_pts, input_bmCodes, input_views, input_uvCodes)`` (models/model.py:121-137) on per-point,
        already-embedded inputs ``[n,input_ch] [n,ch_shape] [n,input_ch_views] [n,ch_tex] -> [n,4]`` (93 / 50 / 27 / 256 at the shipped
        configuration) — the call form of the reference's eager
        ``batchify`` (models/render_class.py:96-109).  Same MFMA layer kernel, weights packed without the constant folding
        (nothing is assumed constant here); the concatenations are free because a panel buffer IS a K-major concat: the
        producer of ``xyz`` / ``sigma`` / ``rgbCodes`` writes behind the code panels of one buffer.  Inference only."""
        L, st = self._L, lib.stream()
        D, W = self.D, self.W
        n = int(pts93.shape[0])
        Wp, Hp = (W + 63) // 64 * 64, (W // 2 + 63) // 64 * 64
        Mp = (n + 255) // 256 * 256
        dev = pts93.device
        packed, biases = self._nominal_pack()
        bim0, bim_skip, uv0, uv_skip, view = 4, 9, 4 + D, 9 + D, 4 + 2 * D
        f = lambda t: t.detach().float().contiguous()
        buf = lambda k: torch.zeros(Mp * k, dtype=torch.float32, device=dev)      # zero: padded rows / columns stay finite

        def to_panels(x, k, dst):
            lib.check(L.mofa_to_panels(lib.ptr(f(x)), n, k, lib.ptr(dst), Mp, st), "mofa_to_panels")

        def layer(li, x1, k1, x2, k2, y, n_pad):
            lib.check(L.mofa_layer_forward(lib.ptr(x1), k1, lib.ptr(x2) if x2 is not None else None, k2, lib.ptr(packed[li]),
                                           lib.ptr(biases[li]), 0, 1, lib.ptr(y), Mp, n_pad, 1, st), "mofa_layer_forward")

        r16 = lambda v_: (v_ + 15) // 16 * 16
        ch_in, cs, ct, cv = int(pts93.shape[-1]), self.ch_shape, self.ch_tex, self.ch_views
        if (ch_in, int(bm50.shape[-1]), int(views27.shape[-1]), int(tex256.shape[-1])) != (self.ch_pe + self.ch_exp, cs, cv, ct):
            raise lib.MofaError(f"NeRF.forward: input widths {ch_in}/{bm50.shape[-1]}/{views27.shape[-1]}/{tex256.shape[-1]} do not match "
                                f"the module's input_ch / input_ch_shapeCodes / input_ch_views / input_ch_textureCodes = "
                                f"{self.ch_pe + self.ch_exp}/{cs}/{cv}/{ct}")
        ks, kt_, kv = r16(cs), r16(ct), r16(cv)
        x93 = buf(r16(ch_in))
        to_panels(pts93, ch_in, x93)
        c_bm, c_tex, c_view = buf(ks + Wp), buf(kt_ + Wp), buf(kv + Wp)          # [code | producer output] concat buffers
        if cs:
            to_panels(bm50, cs, c_bm)
        if ct:
            to_panels(tex256, ct, c_tex)
        to_panels(views27, cv, c_view)
        t = [buf(Wp), buf(Wp)]
        layer(0, x93, r16(ch_in), None, 0, t[0], Wp)
        layer(1, t[0], Wp, None, 0, t[1], Wp)
        layer(2, t[1], Wp, None, 0, t[0], Wp)
        layer(3, t[0], Wp, None, 0, c_bm[ks * Mp:], Wp)                          # xyz_code lands behind the shape-code panels

        def stack(first, skip, cbuf, ck, out):
            layer(first, cbuf, ck + Wp, None, 0, t[0], Wp)
            cur = 0
            for li in range(first + 1, skip):
                layer(li, t[cur], Wp, None, 0, t[cur ^ 1], Wp)
                cur ^= 1
            last = skip + (D - 5) - 1
            for li in range(skip, last + 1):
                dst = out if li == last else t[cur ^ 1]
                if li == skip:
                    layer(li, cbuf, ck + Wp, t[cur], Wp, dst, Wp)
                else:
                    layer(li, t[cur], Wp, None, 0, dst, Wp)
                cur ^= 1

        stack(bim0, bim_skip, c_bm, ks, c_tex[kt_ * Mp:])                        # sigmaCodes land behind the texture-code panels
        stack(uv0, uv_skip, c_tex, kt_, c_view[kv * Mp:])                        # rgbCodes land behind the view-encoding panels
        v = buf(Hp)
        layer(view, c_view, kv + Wp, None, 0, v, Hp)
        raw = torch.empty(n, 4, dtype=torch.float32, device=dev)
        lib.check(L.mofa_head_forward(lib.ptr(c_tex[kt_ * Mp:]), Wp, Mp, lib.ptr(packed[view + 1]), lib.ptr(biases[view + 1]), 1,
                                      lib.ptr(raw), 3, n, st), "mofa_head_forward(alpha)")
        lib.check(L.mofa_head_forward(lib.ptr(v), Hp, Mp, lib.ptr(packed[view + 2]), lib.ptr(biases[view + 2]), 3, lib.ptr(raw), 0, n,
                                      st), "mofa_head_forward(rgb)")
        return raw

    # -- forward -----------------------------------------------------------------------------------
    def forward_rays(self, rays_o, rays_d, z, z_row_stride: int, viewdirs, S: int, raw_out: torch.Tensor,
                     folded: Optional[torch.Tensor] = None, slot: int = 0, snapshot: bool = True, gate: bool = False):
        """raw_out[R,S,4] = NeRF(PE(o + d z), codes, PE(viewdirs)) for R rays x S samples.  ``snapshot=False``: a call on a SIDE
        stream — the caller snapshots the verdict words itself, on the main stream, once it has joined the side streams (two streams
        writing the one pinned mirror could overwrite a raised flag with an older, clean copy).  ``gate=True``: the sigma-gated forward
        (``mofa_net_forward_gated``) — the same sigma everywhere, rgb = 0 where sigma <= 0: for callers that only composite ``raw_out``."""
        R = viewdirs.shape[0]
        if gate:
            return self._forward_gated(rays_o, rays_d, z, z_row_stride, None, viewdirs, R, S, raw_out, folded, slot, snapshot)
        view = self._linears[-3]
        ws = self.workspace(R * S, R, viewdirs.device, slot)
        self.check_verdict()
        lib.check(self._L.mofa_net_forward(self.shape, lib.ptr(self.packed()),
                                           lib.ptr(folded if folded is not None else self._folded),
                                           lib.ptr(view.weight.detach().contiguous()),
                                           lib.ptr(view.bias.detach().contiguous()), lib.ptr(rays_o), lib.ptr(rays_d),
                                           lib.ptr(z), z_row_stride, None, lib.ptr(viewdirs), R, S, lib.ptr(ws),
                                           lib.ptr(raw_out), None, None, None, self.verdict_ptr(viewdirs.device), lib.stream()),
                  "mofa_net_forward")
        if snapshot:
            self.snapshot_verdict()
        return raw_out

    def forward_points(self, pts, viewdirs, S: int, raw_out: torch.Tensor, folded: Optional[torch.Tensor] = None, gate: bool = False):
        """Same with explicit points [R*S,3] (``run_network(inputs, viewdirs, fn)`` entry); ``gate`` as for :meth:`forward_rays`."""
        R = viewdirs.shape[0]
        if gate:
            return self._forward_gated(None, None, None, 0, pts, viewdirs, R, S, raw_out, folded, 0, True)
        view = self._linears[-3]
        ws = self.workspace(R * S, R, viewdirs.device)
        self.check_verdict()
        lib.check(self._L.mofa_net_forward(self.shape, lib.ptr(self.packed()),
                                           lib.ptr(folded if folded is not None else self._folded),
                                           lib.ptr(view.weight.detach().contiguous()),
                                           lib.ptr(view.bias.detach().contiguous()), None, None, None, 0, lib.ptr(pts),
                                           lib.ptr(viewdirs), R, S, lib.ptr(ws), lib.ptr(raw_out), None, None, None,
                                           self.verdict_ptr(viewdirs.device), lib.stream()), "mofa_net_forward")
        self.snapshot_verdict()
        return raw_out

    def density_points(self, pts, sigma_out: torch.Tensor, folded: Optional[torch.Tensor] = None):
        """sigma_out[n] = the pre-ReLU density of the points ``pts [n,3]`` — ``raw[..., 3]`` of :meth:`forward_points` on the same points,
        bit for bit, without the texture stack, the view layer or the rgb head (``mofa_net_density``).  Inference only."""
        n = int(pts.shape[0])
        ws = self.workspace(n, 1, pts.device)
        self.check_verdict()
        lib.check(self._L.mofa_net_density(self.shape, lib.ptr(self.packed()), lib.ptr(folded if folded is not None else self._folded),
                                           lib.ptr(pts), n, lib.ptr(ws), lib.ptr(sigma_out), self.verdict_ptr(pts.device), lib.stream()),
                  "mofa_net_density")
        self.snapshot_verdict()
        return sigma_out
