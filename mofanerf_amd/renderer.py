"""``myRenderer``-compatible volumetric renderer whose hot path runs on hand-written HIP kernels.

Drop-in for ``models/render_class.py:40-437`` of zhuhao-nju/mofanerf: same constructor, same
``render`` / ``render_fitting`` / ``render_path`` / ``run_network`` / ``batchify_rays`` /
``grad_parameter`` surface, same kwargs dict (``create_nerf``'s ``render_kwargs_*``), same return
convention ``[rgb, disp, acc, extras]`` and the same per-call state stored on ``self``.

What runs where
  * HIP (``libmofanerf_hip.so``): ray generation, positional encoding, all 2D+7 layers of both
    networks, sigma/rgb heads, alpha compositing, importance resampling + merge, z_std.
  * PyTorch-ROCm (once per call): ``StyleModule`` on one 50-d row and the texture
    encoder CNN on one 512² map; the handful of elementwise ops that build stochastic sample positions.
There is no eager/CPU fallback: CPU tensors or a missing library raise ``MofaError``.
"""
from __future__ import annotations

import os
import time
from typing import Dict

import numpy as np
import torch

from . import lib
from .autograd import CompositeFn, NetFn, fold_torch, view_bias_torch
from .hipnet import HipNet, unwrap
from .model import EnDeUVmap, StyleModule

_OUT_KEYS = ("rgb_map", "disp_map", "acc_map")


class lossesLog:
    """Accumulator for the texture encoder's auxiliary losses (models/render_class.py:13-37).  The shipped
    encoder returns ``{}``, so :meth:`out` is the int ``0`` — callers add it to the loss (run_train.py:346)."""

    def __init__(self, lossesList, Weight):
        self.lossesNameList = list(lossesList)
        self.lossesWeight = dict(zip(lossesList, Weight))
        self.lossesDict = {n: 0 for n in lossesList}
        self.chunkDict = {n: 0 for n in lossesList}

    def update(self, lossesList, chunk):
        for name, value in lossesList.items():
            self.lossesDict[name] = self.lossesDict[name] + torch.sum(value)
            self.chunkDict[name] += chunk

    def out(self):
        loss = 0
        for name in self.lossesNameList:
            if not (isinstance(self.lossesDict[name], int) and self.lossesDict[name] == 0):
                loss = loss + self.lossesDict[name] / self.chunkDict[name] * self.lossesWeight[name]
            self.lossesDict[name], self.chunkDict[name] = 0, 0
        return loss


# The reference's own use_viewdirs=False branch cannot execute: NeRF.forward (models/model.py:121-137) uses alpha_linear / rgb_linear,
# which exist only when use_viewdirs=True (:104-110 builds output_linear instead), and run_network (models/render_class.py:86-92)
# then hands `batchify` two inputs where its `v1, v2, v3 = inputs` (:101) needs three.  There is no behaviour to be equal to, so
# the flag is rejected up front — with the reason — instead of failing deep inside a kernel launch.
_NO_VIEWDIRS = ("use_viewdirs=False: the reference's own path for it cannot run (models/model.py:121-137 needs alpha_linear / "
                "rgb_linear, created only for use_viewdirs=True; models/render_class.py:101 unpacks three network inputs), and every "
                "shipped config sets use_viewdirs=True (configs/exp_mofanerf.txt)")


def _scalar(v) -> float:
    return float(v.item() if torch.is_tensor(v) else v)


class Renderer(torch.nn.Module):
    def __init__(self, embed_fn=None, embeddirs_fn=None, netchunk=1024 * 64, uvCodesLen=256, expCodesLen=4,
                 input_ch=3, shapeCodes=50):
        super().__init__()
        # embed_fn / embeddirs_fn (get_embedder's objects): the encoding itself is fused into the first-layer kernel; what the
        # renderer takes from them is HOW MANY frequencies they encode (multires / multires_views, tools/config_parser.py:51-56),
        # which it hands to the C plan.  None = the shipped 10 / 4.
        self.embed_fn, self.embeddirs_fn = embed_fn, embeddirs_fn
        self.point_freqs = self._freqs(embed_fn, 10, "embed_fn")
        self.view_freqs = self._freqs(embeddirs_fn, 4, "embeddirs_fn")
        self.netchunk = netchunk
        self.texEncoder = EnDeUVmap(uvCodesLen)
        self.lossList = ["loss_deformReg", "loss_kldiv", "loss_offsets"]
        self.lossWeight = [0.05, 1, 0.01]
        self.lossLog = lossesLog(self.lossList, self.lossWeight)
        self.idSpecificMod = StyleModule()
        self.is_run_fineNet = True
        self.expCodes_Sigma = [torch.rand([1, expCodesLen]) for _ in range(20)]   # 20 kinds of expression
        for latent in self.expCodes_Sigma:
            latent.requires_grad = True
        self._hipnets: Dict[int, HipNet] = {}
        self._L = None
        # render() (training entry) back-propagates into the network weights; render_fitting() optimises only codes /
        # pose / light, so by default it skips the weight-gradient GEMMs the reference computes and throws away
        # (run_fit.py never steps the networks); set fit_weight_grads=True to populate weight.grad there too
        self.fit_weight_grads = False
        self._weight_grads = False
        # what a fitting step (no weight gradients) keeps for its backward: "mask" = one bit per activation (all it needs; 1/32 of the
        # fp32 tape, bit-identical gradients), "fp32" = every layer output (the A/B arm; what a step WITH weight gradients always keeps)
        self.fit_tape = os.environ.get("MOFA_FIT_TAPE", "mask")
        self._tex_cache = None
        self._cache: Dict[tuple, torch.Tensor] = {}
        # training / fitting memory: False (default) keeps every layer output of every sub-batch for the backward (nothing is
        # recomputed: 98 KiB per fine-network point, 52.6 GB at N_rand = 4096 — sized for 288 GB); True keeps only the inputs and
        # re-runs each sub-batch's forward inside its backward (autograd.NetFn): one sub-batch's tape at a time, bit-identical gradients,
        # one extra forward pass per step.  MOFA_TAPE=recompute sets it for every renderer.
        self.tape_recompute = os.environ.get("MOFA_TAPE", "") == "recompute"
        self.n_streams = int(os.environ.get("MOFA_STREAMS", "1"))   # concurrent sub-batches of the inference path (render_rays)
        self._streams = {}
        self.png_sink = None      # optional mofanerf_amd.io.PngSink shared by consecutive render_path calls (bulk renders)
        self.mesh_stats = None    # the statistics of the last narrow-band extract_mesh (mesh.band_surface's, plus "edge_ids") or refined one ("refine", "zero_normals") or filtered one ("components")
        self.occupancy_stats = None   # the last render* call with an occupancy grid: {"coarse" / "fine": {"samples", "kept"}}, summed over chunks

    @staticmethod
    def _freqs(fn, default, what):
        """Number of encoding frequencies of a ``get_embedder`` result (models/model.py:48-63): ``Embedder.n_freqs``; ``nn.Identity``
        (i_embed = -1) encodes nothing: 0; ``None``: the shipped default.  Any other callable is refused — the kernel generates the
        encoding itself and would silently disagree with an encoder it cannot see into."""
        if fn is None:
            return default
        if isinstance(fn, torch.nn.Identity):
            return 0
        n = getattr(fn, "n_freqs", None)
        if n is None:
            raise lib.MofaError(f"{what} must come from mofanerf_amd.embedder.get_embedder (or be None / nn.Identity): the positional "
                                "encoding is generated inside the first-layer kernel from its frequency count")
        return int(n)

    def _side_streams(self, n, dev):
        key = (str(dev), n)
        if key not in self._streams:
            self._streams[key] = [torch.cuda.Stream(device=dev) for _ in range(n)]
        return self._streams[key]

    # expCodes_Sigma is a plain list (not registered parameters, render_class.py:53-58): move it with the module
    # — IN PLACE, the way nn.Module moves parameters: the tensor OBJECTS survive .cuda()/.to()/.float(), so an optimizer or
    # `grad_vars` built before the move (create_nerf builds them, run_fit.py:175 then calls render.cuda()) keeps training them
    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        with torch.no_grad():
            for t in self.expCodes_Sigma:
                t.data = fn(t.data)
                if t.grad is not None:
                    t.grad.data = fn(t.grad.data)
        self._cache.clear()
        return self

    def invalidate_caches(self):
        """Drop every derived device-side copy: packed / transposed weight panels of both networks, the cached
        texture code and the constant sample rows.  The caches are keyed on ``(data_ptr, tensor._version)``, which every
        autograd-visible in-place update bumps (optimizer steps, ``load_state_dict``, ``copy_``) — but an edit made THROUGH
        ``.data`` (``w.data.copy_(...)``, ``w.data[:] = ...``) does not, so call this after one."""
        for h in self._hipnets.values():
            h.invalidate()
        self._tex_cache = None
        self._cache.clear()

    def grad_parameter(self):
        grad_vars = list(self.expCodes_Sigma)
        if self.texEncoder is not None:
            grad_vars += list(self.texEncoder.parameters())
        if self.idSpecificMod is not None:
            grad_vars += list(self.idSpecificMod.parameters())
        return grad_vars

    # ------------------------------------------------------------------------------------------------
    def _lib(self):
        if self._L is None:
            self._L = lib.load()
        return self._L

    def _hip(self, net) -> HipNet:
        net = unwrap(net)
        h = self._hipnets.get(id(net))
        if h is None or h.net is not net or h.point_freqs != self.point_freqs or h.view_freqs != self.view_freqs:
            h = HipNet(net, point_freqs=self.point_freqs)
            if h.view_freqs != self.view_freqs:       # (checked BEFORE the entry is cached: a refused network is refused every time)
                raise lib.MofaError(f"NeRF.input_ch_views = {net.input_ch_views} (multires_views = {h.view_freqs}) but the renderer's "
                                    f"embeddirs_fn encodes {self.view_freqs} frequencies (tools/create_model_condition.py:16-22 builds "
                                    "both from args.multires_views)")
            self._hipnets[id(net)] = h
        return h

    def _device(self):
        return next(self.idSpecificMod.parameters()).device

    def bind(self, *nets):
        """Create the device-side state of ``nets`` (``HipNet``: the plan check against the module, ``mofa_device_init``'s per-device
        census — the library's one synchronising call) up front, so that the first ``render()`` finds everything in place;
        ``create_nerf`` calls it.  Networks that were not bound are bound at their first use."""
        for n in nets:
            if n is not None:
                self._hip(n)
        return self

    def frame_check(self):
        """A callable that waits for the launches issued SO FAR on the current stream and raises ``MofaError`` if one of them was a
        chained launch that ended incomplete — safe to run on another thread (the PNG sink's workers; ``HipNet.verdict_token``)."""
        looks = [t for t in (h.verdict_token() for h in list(self._hipnets.values())) if t is not None]

        def check():
            for look in looks:
                look()
        return check

    def gate_stats(self, reset: bool = False):
        """Samples and live samples (raw sigma not <= 0) of the sigma-gated forwards so far, per bound network: ``{(D, W): {"samples",
        "live"}}``.  Reads device-side accumulators (one host synchronisation, here and nowhere on the render path): for tools."""
        out = {}
        for h in list(self._hipnets.values()):
            if h.gate_stats_dev is not None:
                n, live = (int(v) for v in h.gate_stats_dev.tolist())
                out[(h.D, h.W)] = {"samples": n, "live": live}
                if reset:
                    h.gate_stats_dev.zero_()
        return out

    def check_launches(self, block: bool = True):
        """Raise ``MofaError`` if any chained launch issued through this renderer ended incomplete (the kernel abandons a launch rather
        than compute on incomplete inputs, and a verification kernel then overwrites the outputs with NaN — see
        ``HipNet.check_verdict``).  The launch paths look without blocking before every call; ``block=True`` waits for the verdict of
        everything issued so far — for whoever consumes a frame (``render_path`` after its copies, the PNG sink, bench, tests)."""
        for h in list(self._hipnets.values()):
            h.check_verdict(block=block)

    def _const_row(self, key, builder, device):
        """Small per-call constant rows (sample positions, u) are built once on the host with the same torch CPU
        ops as the reference and cached on the device."""
        k = (key, str(device))
        if k not in self._cache:
            row = builder().float().contiguous()
            # through pinned memory, asynchronously: a pageable host->device copy synchronises the host, and the first frame of a
            # process must not (eight ranks would each stall); the stream orders the copy before the kernels that read the row
            self._cache[k] = row.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else row.to(device)
        return self._cache[k]

    def _fold_codes(self, net, tex_code):
        """Per-call conditioning: e = scale*sigma[expType] + bias (render_class.py:75-82) and the folded biases.
        With autograd enabled the (tiny, per-call) fold is a differentiable torch expression so that gradients reach the
        codes; otherwise it is the HIP kernel."""
        style = unwrap(self.idSpecificMod)
        row = self.shapeCodes[0, :].reshape(1, -1).float().to(self._device())
        scale, bias = style(row)
        e = scale * self.expCodes_Sigma[self.expType].to(row.device) + bias
        if torch.is_grad_enabled():
            # fitting (no weight gradients requested): the fold uses DETACHED weights and biases, so gradients reach the codes
            # and the pose only and no network parameter ever receives a partial .grad (it stays None)
            return fold_torch(self._hip(net), e, row, tex_code.to(row.device).float(), detach_params=not self._weight_grads)
        return self._hip(net).fold(e, row, tex_code.to(row.device))

    # ------------------------------------------------------------------------------------------------
    def run_network(self, inputs, viewdirs, fn=None, weight_grads=None):
        """``inputs [R,S,3]`` points, ``viewdirs [R,3]`` -> raw ``[R,S,4]`` (render_class.py:69-94; also ``network_query_fn``,
        tools/create_model_condition.py:50).  Under autograd it is differentiable like the reference's: gradients reach
        ``inputs``, ``viewdirs``, the shape / texture / expression codes (through ``self.shapeCodes``, ``self.decoding_texCodes``,
        ``self.expCodes_Sigma``) and the StyleModule — HIP backward (``mofa_net_backward`` with explicit points).  The network WEIGHTS
        take part exactly as in an autograd graph: ``weight_grads=None`` (default) = those that ``requires_grad`` — a property of the
        call's arguments alone, not of whatever ``render()`` / ``render_fitting()`` ran before it (round 5 defaulted to the last
        entry point's choice: call-history-dependent); ``False`` leaves them out (a fitting loop that never steps the networks saves
        the weight-gradient GEMMs and the fp32 tape), ``True`` is the same as ``None``.  The tape-keeping path is taken only if
        something actually asks for a gradient: a plain call outside ``no_grad`` whose inputs, codes and (participating) weights all
        have ``requires_grad=False`` runs the inference kernels and keeps nothing."""
        if viewdirs is None:
            raise NotImplementedError(_NO_VIEWDIRS)
        R, S = int(inputs.shape[0]), int(inputs.shape[1])
        h = self._hip(fn)
        want_w = (weight_grads is None or bool(weight_grads)) and any(l.weight.requires_grad or l.bias.requires_grad for l in h._linears)
        needs_grad = torch.is_grad_enabled() and (want_w or self._asks_grad(inputs, viewdirs))
        keep, self._weight_grads = self._weight_grads, want_w
        try:
            with torch.set_grad_enabled(needs_grad):
                folded = self._fold_codes(fn, self.decoding_texCodes)
        finally:
            self._weight_grads = keep
        rays_per = max(1, int(self.netchunk) // S)
        if needs_grad:
            h.tape_recompute, h.force_fp32_tape = bool(self.tape_recompute), self.fit_tape == "fp32"
            pts = inputs.reshape(-1, 3).float()
            vb = view_bias_torch(h, viewdirs.float(), detach_params=not want_w)
            wts = [l.weight for l in h._linears] if want_w else []
            parts = [NetFn.apply(h, None, None, None, 0, S, folded, vb[i:i + rays_per], pts[i * S:(i + rays_per) * S], *wts)
                     for i in range(0, R, rays_per)]
            return parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        raw = torch.empty(R, S, 4, dtype=torch.float32, device=inputs.device)
        pts = inputs.detach().reshape(-1, 3).float().contiguous()
        vd = viewdirs.detach().float().contiguous()
        for i in range(0, R, rays_per):
            j = min(R, i + rays_per)
            h.forward_points(pts[i * S:j * S], vd[i:j], S, raw[i:j], folded)
        return raw

    def batchify(self, fn, chunk):
        """The reference's eager helper (models/render_class.py:96-109): a version of ``fn`` applied to ``chunk``-sized slices of
        already-embedded inputs ``[embedded93, shapeCodes, embedded_dirs]`` (+ the expanded texture code).  ``fn`` is a ``NeRF``
        (its ``forward`` runs the HIP layer kernels on embedded inputs).  The renderer itself does not use it — ``run_network``
        fuses embedding, code folding and sub-batching — it exists so that code written against the reference keeps working."""
        fn = unwrap(fn)
        if chunk is None:
            return fn

        def ret(inputs):
            v1, v2, v3 = inputs
            t = self.decoding_texCodes.reshape(1, -1).expand(v1.shape[0], -1)
            return torch.cat([fn(v1[i:i + chunk], v2[i:i + chunk], v3[i:i + chunk], t[i:i + chunk])
                              for i in range(0, v1.shape[0], chunk)], 0)

        return ret

    def batchify_rays(self, chunk=1024 * 32, **kwargs):
        """Render ``self.rays`` in chunks of ``chunk`` rays (render_class.py:111-123)."""
        all_ret: Dict[str, list] = {}
        direct = getattr(self, "_rays_ref", None) is not self.rays
        if direct:      # called on a caller-built self.rays: fold the per-call codes ONCE for all chunks (render_rays alone folds per call)
            self._fold_direct(kwargs.get("network_fn"), kwargs.get("network_fine"))
            self._folds_hoisted = True
        try:
            for i in range(0, self.rays.shape[0], chunk):
                ret = self.render_rays([i, i + chunk], **kwargs)
                for k, v in ret.items():
                    all_ret.setdefault(k, []).append(v)
        finally:
            self._folds_hoisted = False
        return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}

    def _fold_direct(self, network_fn, network_fine):
        self._folded_coarse = self._fold_codes(network_fn, self.decoding_texCodes).clone()
        self._folded_fine = self._fold_codes(network_fine, self.decoding_texCodes).clone() if network_fine is not None else None

    # ---- the sampling schedule of a chunk of R rays, shared by render_rays and render_geometry ---------------------------------------
    # Its random draws are behaviour: t_rand [R,S] here, u [R,Ni] in _importance_positions (render_rays draws its raw noise between and
    # after them), each `pytest` draw behind its own np.random.seed(0).
    def _coarse_positions(self, near, far, R, S, lindisp, perturb, pytest, dev):
        """The coarse sample positions ``(z, z_stride)`` (render_class.py:266-287).  ``near`` / ``far``: two floats — one row shared by
        every ray (``z_stride = 0``), built on the host as the reference builds it and cached — or two per-ray ``[R,1]`` columns."""
        t_row = self._const_row(("t", S), lambda: torch.linspace(0., 1., steps=S), dev)
        if not torch.is_tensor(near):
            def z_row():
                t = torch.linspace(0., 1., steps=S)
                n, f = torch.tensor([[near]]), torch.tensor([[far]])
                z = n * (1. - t) + f * t if not lindisp else 1. / (1. / n * (1. - t) + 1. / f * t)
                return z.reshape(-1)

            z, z_stride = self._const_row(("z", near, far, S, bool(lindisp)), z_row, dev), 0
        else:
            z = (near * (1. - t_row) + far * t_row if not lindisp else 1. / (1. / near * (1. - t_row) + 1. / far * t_row)).contiguous()
            z_stride = S
        if perturb > 0.:
            zz = z[None, :].expand(R, S) if z_stride == 0 else z
            mids = .5 * (zz[..., 1:] + zz[..., :-1])
            upper, lower = torch.cat([mids, zz[..., -1:]], -1), torch.cat([zz[..., :1], mids], -1)
            if pytest:
                np.random.seed(0)
                t_rand = torch.Tensor(np.random.rand(R, S)).to(dev)
            else:
                t_rand = torch.rand(R, S, device=dev)
            z, z_stride = (lower + (upper - lower) * t_rand).contiguous(), S
        return z, z_stride

    def _importance_positions(self, z, z_stride, weights, R, S, Ni, perturb, pytest, dev):
        """``(z_samples [R,Ni], z_fine [R,S+Ni], z_std [R])`` from the coarse pass's weights: ``mofa_sample_pdf_merge``."""
        if perturb == 0.:            # det=(perturb == 0.), render_class.py:325
            u, u_stride = self._const_row(("u", Ni), lambda: torch.linspace(0., 1., steps=Ni), dev), 0
        elif pytest:
            np.random.seed(0)
            u, u_stride = torch.Tensor(np.random.rand(R, Ni)).to(dev).contiguous(), Ni
        else:
            u, u_stride = torch.rand(R, Ni, device=dev), Ni
        z_samples = torch.empty(R, Ni, dtype=torch.float32, device=dev)
        z_fine = torch.empty(R, S + Ni, dtype=torch.float32, device=dev)
        z_std = torch.empty(R, dtype=torch.float32, device=dev)
        # z_samples are detached in the reference (render_class.py:326): no gradient through the resampling
        lib.check(self._lib().mofa_sample_pdf_merge(lib.ptr(z), z_stride, lib.ptr(weights.detach()), lib.ptr(u), u_stride, R, S, Ni,
                                                    lib.ptr(z_samples), lib.ptr(z_fine), lib.ptr(z_std), lib.stream()), "mofa_sample_pdf_merge")
        return z_samples, z_fine, z_std

    def _culled_pass(self, occupancy, which, rays_o, rays_d, zv, zs, n_s):
        """Classify and compact one pass's samples (``occupancy.CulledPass``: one host read, the kept count) and add them to
        ``self.occupancy_stats[which]``."""
        from .occupancy import CulledPass
        cp = CulledPass(occupancy, rays_o, rays_d, zv, zs, n_s)
        stats = self.occupancy_stats.setdefault(which, {"samples": 0, "kept": 0})
        stats["samples"] += cp.n_samples
        stats["kept"] += cp.n_kept
        return cp

    @staticmethod
    def _bounds(near, far, rays_d):
        """``near`` / ``far``, each a scalar (the shipped call sites) or a per-ray array, as render_class.py:174 broadcasts it: two floats
        (the scalar fast path), or — when either is per ray — two ``[R,1]`` columns beside ``rays_d [R,3]``."""
        per_ray = lambda v: torch.is_tensor(v) and v.numel() > 1 or isinstance(v, np.ndarray) and v.size > 1
        if not per_ray(near) and not per_ray(far):
            return _scalar(near), _scalar(far)
        ones = torch.ones_like(rays_d[..., :1])
        return tuple(torch.as_tensor(v, dtype=torch.float32).reshape(-1, 1).to(ones.device) * ones if per_ray(v) else _scalar(v) * ones
                     for v in (near, far))

    # ------------------------------------------------------------------------------------------------
    def render_rays(self, ray_batch, network_fn, N_samples, retraw=False, lindisp=False, perturb=0., N_importance=0,
                    network_fine=None, white_bkgd=False, raw_noise_std=0., network_query_fn=None, verbose=False,
                    pytest=False, occupancy=None):
        """Coarse + fine volumetric rendering of rays ``self.rays[b0:b1]`` (render_class.py:239-352).

        ``occupancy`` (an ``occupancy.OccupancyGrid``, from :meth:`build_occupancy` or ``occupancy_from_grid``): occupancy-culled
        rendering — in each pass the network runs only on the samples whose point lies in an occupied cell of the grid (explicit
        points through ``mofa_net_forward``, in sub-batches of ``netchunk`` points); every other sample gets ``raw = (0,0,0,0)``, hence
        ``alpha = 0`` and weight 0 exactly.  The frame equals, bit for bit, the un-culled pipeline with those samples' raw values
        replaced by zero; compositing and the importance resampling are unchanged.  Everything outside the grid's bounds is empty.  The
        grid lives in the space of the points the network is given: with ``ndc=True`` those are NDC points, so the grid's bounds must be
        NDC bounds (no conversion is done); the face scripts render with ``ndc=False``.  Inference only (a tensor that asks for a
        gradient under ``torch.is_grad_enabled()`` is refused) and ``raw_noise_std`` must be 0.  Each pass reads its kept count back to the
        host (one synchronisation per pass and chunk of rays); ``self.occupancy_stats`` sums samples and kept samples per pass.
        ``None`` (default): nothing changes."""
        L = self._lib()
        rays = self.rays[ray_batch[0]:ray_batch[1]]
        R, dev = int(rays.shape[0]), rays.device
        if rays.shape[-1] <= 8:
            raise NotImplementedError(_NO_VIEWDIRS)
        rays_o, rays_d, vd = (rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), rays[:, 8:11].contiguous())
        S = int(N_samples)      # any count: up to 256 samples a ray is one pass of its wavefront, beyond that the kernels walk passes
        st = lib.stream()
        # near / far: the scalar fast path when render()/render_fitting() set them for THIS self.rays; otherwise (per-ray
        # bounds, or batchify_rays()/render_rays() called directly on a caller-built self.rays) they are read from columns 6:8
        # (an in-place edit of self.rays after render() — e.g. per-ray bounds written into columns 6:8 — bumps its version counter and
        #  drops the scalar fast path: the columns are what the reference's render_rays reads, models/render_class.py:262-264)
        scalar_bounds = (getattr(self, "_rays_ref", None) is self.rays and self._near is not None
                         and self.rays._version == getattr(self, "_rays_version", -1))
        near, far = (self._near, self._far) if scalar_bounds else (rays[:, 6:7], rays[:, 7:8])
        z, z_stride = self._coarse_positions(near, far, R, S, lindisp, perturb, pytest, dev)

        def noise_for(n_s):
            if not raw_noise_std > 0.:
                return None
            if pytest:
                np.random.seed(0)
                return torch.Tensor(np.random.rand(R, n_s) * raw_noise_std).to(dev).contiguous()
            return (torch.randn(R, n_s, device=dev) * raw_noise_std).contiguous()

        grad = torch.is_grad_enabled()
        # the sigma-gated forward (colour half only where sigma > 0): whenever nothing but compositing reads raw — noise would change
        # which samples are dead, and retraw hands raw to the caller
        gate = not grad and not raw_noise_std > 0. and not retraw

        def composite(raw, zv, zs, n_s, noise):
            if grad:
                rgb, disp, acc, depth, weights = CompositeFn.apply(raw, zv, zs, rays_d, noise, bool(white_bkgd))
                return {"rgb": rgb, "disp": disp, "acc": acc, "depth": depth, "weights": weights}
            o = {k: torch.empty(R, *sh, dtype=torch.float32, device=dev)
                 for k, sh in (("rgb", (3,)), ("disp", ()), ("acc", ()), ("depth", ()), ("weights", (n_s,)))}
            lib.check(L.mofa_composite_forward(lib.ptr(raw), lib.ptr(zv), zs, lib.ptr(rays_d), lib.ptr(noise), R, n_s,
                                               int(bool(white_bkgd)), lib.ptr(o["rgb"]), lib.ptr(o["disp"]),
                                               lib.ptr(o["acc"]), lib.ptr(o["depth"]), lib.ptr(o["weights"]), st),
                      "mofa_composite_forward")
            return o

        def network(net, folded, zv, zs, n_s):
            h = self._hip(net)
            rays_per = max(1, int(self.netchunk) // n_s)
            if grad:     # tape-keeping forward per sub-batch; the per-ray view bias is a differentiable torch expression
                h.tape_recompute, h.force_fp32_tape = bool(self.tape_recompute), self.fit_tape == "fp32"
                vb = view_bias_torch(h, vd, detach_params=not self._weight_grads)
                wts = [l.weight for l in h._linears] if self._weight_grads else []
                parts = [NetFn.apply(h, rays_o[i:i + rays_per], rays_d[i:i + rays_per],
                                     zv[i:i + rays_per] if zs else zv, zs, n_s, folded, vb[i:i + rays_per], None, *wts)
                         for i in range(0, R, rays_per)]
                return parts[0] if len(parts) == 1 else torch.cat(parts, 0)
            raw = torch.empty(R, n_s, 4, dtype=torch.float32, device=dev)
            starts = list(range(0, R, rays_per))
            n_str = min(self.n_streams, len(starts))
            if n_str <= 1:
                for i in starts:
                    j = min(R, i + rays_per)
                    h.forward_rays(rays_o[i:j], rays_d[i:j], zv[i:j] if zs else zv, zs, vd[i:j], n_s, raw[i:j], folded, gate=gate)
                return raw
            # Independent sub-batches round-robin over a few streams: kernels of different streams are not in step with each
            # other, so one stream's launch boundaries (tail, write burst, first fetches) are filled by the others' workgroups.
            h.packed()                                              # (re)pack on the main stream, before the side streams fork
            if gate:
                h.gate_stats_buffer(dev)                            # (likewise: created and zeroed before any side stream adds to it)
            main = torch.cuda.current_stream(dev)
            side = self._side_streams(n_str, dev)
            for s_ in side:
                s_.wait_stream(main)
            for k, i in enumerate(starts):
                j = min(R, i + rays_per)
                with torch.cuda.stream(side[k % n_str]):
                    h.forward_rays(rays_o[i:j], rays_d[i:j], zv[i:j] if zs else zv, zs, vd[i:j], n_s, raw[i:j], folded,
                                   slot=k % n_str, snapshot=False, gate=gate)
            for s_ in side:
                main.wait_stream(s_)
            h.snapshot_verdict()       # ONE snapshot, on the main stream, behind every side stream's launches
            return raw

        def network_culled(net, folded, zv, zs, n_s, which):
            # classify, compact (one host read: n_kept), network on the kept samples as explicit points with one view direction each
            # (S = 1), scatter: every element of raw is written by the scatter kernel
            h = self._hip(net)
            cp = self._culled_pass(occupancy, which, rays_o, rays_d, zv, zs, n_s)
            raw = torch.empty(R, n_s, 4, dtype=torch.float32, device=dev)
            raw_kept = None
            if cp.n_kept:
                pts, dirs, _ = cp.gather(vd)
                raw_kept = torch.empty(cp.n_kept, 1, 4, dtype=torch.float32, device=dev)
                per = max(1, int(self.netchunk))
                for i in range(0, cp.n_kept, per):
                    h.forward_points(pts[i:i + per], dirs[i:i + per], 1, raw_kept[i:i + per], folded, gate=gate)
            return cp.scatter(raw_kept, raw)

        if occupancy is not None:
            self._check_occupancy(occupancy, rays, raw_noise_std, network_fn, network_fine)
            if self.occupancy_stats is None:
                self.occupancy_stats = {}
        if getattr(self, "_rays_ref", None) is not self.rays and not getattr(self, "_folds_hoisted", False):
            # called directly on a caller-built self.rays (the reference documents batchify_rays / render_rays as callable once
            # self.rays, shapeCodes, expType and decoding_texCodes are set): fold the per-call codes here (batchify_rays hoists it)
            self._fold_direct(network_fn, network_fine)
        raw = (network(network_fn, self._folded_coarse, z, z_stride, S) if occupancy is None else
               network_culled(network_fn, self._folded_coarse, z, z_stride, S, "coarse"))
        c = composite(raw, z, z_stride, S, noise_for(S))
        ret = {"rgb_map": c["rgb"], "disp_map": c["disp"], "acc_map": c["acc"]}

        if N_importance > 0 and self.is_run_fineNet:
            Ni = int(N_importance)
            z_samples, z_fine, z_std = self._importance_positions(z, z_stride, c["weights"], R, S, Ni, perturb, pytest, dev)
            fine = network_fn if network_fine is None else network_fine
            folded = self._folded_coarse if network_fine is None else self._folded_fine
            raw = (network(fine, folded, z_fine, S + Ni, S + Ni) if occupancy is None else
                   network_culled(fine, folded, z_fine, S + Ni, S + Ni, "fine"))
            f = composite(raw, z_fine, S + Ni, S + Ni, noise_for(S + Ni))
            ret = {"rgb_map": f["rgb"], "disp_map": f["disp"], "acc_map": f["acc"], "rgb0": c["rgb"],
                   "disp0": c["disp"], "acc0": c["acc"], "z_std": z_std}
            if verbose:
                ret["_z_samples"], ret["_z_fine"], ret["_weights0"] = z_samples, z_fine, c["weights"]
                ret["_z_coarse"] = z if z_stride else z[None, :].expand(R, S)
        if retraw:
            ret["raw"] = raw
        return ret

    def _check_occupancy(self, occupancy, rays, raw_noise_std, network_fn, network_fine):
        """The refusals of occupancy-culled rendering (render_rays): each names its argument."""
        from .occupancy import OccupancyGrid
        if not isinstance(occupancy, OccupancyGrid):
            raise lib.MofaError(f"occupancy: want an occupancy.OccupancyGrid (Renderer.build_occupancy / occupancy_from_grid), got "
                                f"{type(occupancy).__name__}")
        if not rays.is_cuda:
            raise lib.MofaError("occupancy: the rays are CPU tensors; there is no CPU path")
        if occupancy.device != rays.device:
            raise lib.MofaError(f"occupancy: the grid lives on {occupancy.device}, the rays on {rays.device}")
        if raw_noise_std > 0.:
            raise lib.MofaError(f"raw_noise_std = {raw_noise_std} with occupancy: noise would give the skipped samples a density; "
                                "culled rendering is for inference (raw_noise_std = 0)")
        if torch.is_grad_enabled():
            nets = [unwrap(n) for n in (network_fn, network_fine) if n is not None]
            if self._asks_grad(rays) or (self._weight_grads and any(q.requires_grad for n in nets for q in n.parameters())):
                raise lib.MofaError("occupancy: culled rendering is inference only, but autograd is enabled and a tensor (rays, codes, "
                                    "StyleModule or network weights) asks for a gradient; render under torch.no_grad()")

    def _asks_grad(self, *tensors):
        """Whether one of ``tensors``, of this call's codes or of the StyleModule's parameters asks for a gradient."""
        rg = lambda t: torch.is_tensor(t) and t.requires_grad
        return (any(rg(t) for t in tensors) or rg(self.shapeCodes) or rg(self.decoding_texCodes) or rg(self.expCodes_Sigma[self.expType]) or
                any(q.requires_grad for q in unwrap(self.idSpecificMod).parameters()))

    # ------------------------------------------------------------------------------------------------
    def _make_rays(self, H, W, K, c2w, rays, use_viewdirs, c2w_staticcam, ndc):
        if not use_viewdirs:
            raise NotImplementedError(_NO_VIEWDIRS)
        L, dev = self._lib(), self._device()
        if dev.type != "cuda":
            raise lib.MofaError("the renderer must be on the GPU (render.cuda()); there is no CPU path")

        def gen(pose):
            n = int(H) * int(W)
            o, d = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(2))
            if torch.is_tensor(pose):        # stays on the device when it is there already: no device->host->device hop, no host sync
                pose_t = pose.detach()[:3, :4].to(device=dev, dtype=torch.float32).contiguous()
            else:
                pose_t = torch.as_tensor(np.asarray(pose), dtype=torch.float32)[:3, :4].contiguous().to(dev)
            lib.check(L.mofa_get_rays(int(H), int(W), _scalar(K[0][0]), _scalar(K[1][1]), _scalar(K[0][2]),
                                      _scalar(K[1][2]), lib.ptr(pose_t), 0, n, lib.ptr(o), lib.ptr(d), None,
                                      lib.stream()), "mofa_get_rays")
            return o, d

        if c2w is not None:
            rays_o, rays_d = gen(c2w)
            sh = (int(H), int(W), 3)
        else:
            rays_o, rays_d = rays[0], rays[1]
            sh = tuple(rays_d.shape)
            rays_o = rays_o.reshape(-1, 3).float().to(dev)       # may carry gradients to the camera pose (run_fit.py:281)
            rays_d = rays_d.reshape(-1, 3).float().to(dev)
        # ONE statement of the view directions, the reference's (render_class.py:399-401), for a pose and for given rays alike: a frame
        # rendered from a pose is, bit for bit, the frame rendered from that pose's rays (mofa_get_rays' own viewdirs output is the
        # correctly rounded rd / sqrt((x^2 + y^2) + z^2), up to 2 ulp from what torch.norm gives on the device)
        viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        if c2w_staticcam is not None:      # visualise the effect of viewdirs only (render_class.py:161-163)
            rays_o, rays_d = gen(c2w_staticcam)
        if ndc:                            # forward-facing scenes (render_class.py:166-169); viewdirs stay the world-space ones
            from .rays import ndc_rays
            rays_o, rays_d = ndc_rays(int(H), int(W), _scalar(K[0][0]), 1., rays_o, rays_d)
            rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        return rays_o, rays_d, viewdirs, sh

    def _render_common(self, H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, tex_code, kwargs):
        kwargs = dict(kwargs)
        kwargs.pop("network_query_fn", None)
        rays_o, rays_d, viewdirs, sh = self._make_rays(H, W, K, c2w, rays, use_viewdirs, c2w_staticcam, ndc)
        near, far = self._bounds(near, far, rays_d)
        if torch.is_tensor(near):       # per ray: render_rays reads them from columns 6:8
            self._near = self._far = None
        else:
            ones = torch.ones_like(rays_d[..., :1])
            self._near, self._far, near, far = near, far, near * ones, far * ones
        self.rays = torch.cat([rays_o, rays_d, near, far, viewdirs], -1)
        self._rays_ref = self.rays          # (a reference, not an id: ids are reused after garbage collection)
        self._rays_version = self.rays._version
        self.decoding_texCodes = tex_code
        self.occupancy_stats = None
        # inference (torch.no_grad(), as the reference's render-only call sites run): pure HIP, nothing recorded;
        # with autograd enabled (fitting / training) the tape-keeping forward + HIP backward path is used
        self._folded_coarse = self._fold_codes(kwargs["network_fn"], tex_code).clone()
        fine = kwargs.get("network_fine")
        self._folded_fine = self._fold_codes(fine, tex_code).clone() if fine is not None else None
        all_ret = self.batchify_rays(chunk, **kwargs)
        for k in all_ret:
            all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
        ret_list = [all_ret[k] for k in _OUT_KEYS]
        ret_dict = {k: all_ret[k] for k in all_ret if k not in _OUT_KEYS}
        if self.lossList is not None:
            ret_dict["losses"] = self.lossLog.out()
        return ret_list + [ret_dict]

    def render(self, H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, shapeCodes=None, uvMap=None,
               expType=None, near=0., far=1., use_viewdirs=False, c2w_staticcam=None, **kwargs):
        """Training / bulk-render entry: the texture code comes from the encoder CNN on ``uvMap [512,512,3]``
        (render_class.py:125-197)."""
        self.shapeCodes, self.uvMap = shapeCodes, uvMap
        self.expType = int(expType)
        self._weight_grads = True
        enc = unwrap(self.texEncoder)
        if torch.is_grad_enabled():
            code, enlosses = enc(uvMap.permute([2, 0, 1]).unsqueeze(0), self.lossList)
        else:
            # render-only (bulk rendering shows the same UV map for every expression/view of an identity,
            # render_refine_trainSet.py:288-289): the code is cached per (map storage, map version, encoder weights)
            key = (uvMap.data_ptr(), uvMap._version, tuple(uvMap.shape)) + tuple((p.data_ptr(), p._version) for p in enc.parameters())
            if self._tex_cache is None or self._tex_cache[0] != key:
                code, enlosses = enc(uvMap.permute([2, 0, 1]).unsqueeze(0), self.lossList)
                self._tex_cache = (key, code, enlosses)
            _, code, enlosses = self._tex_cache
        self.lossLog.update(enlosses, 1)
        return self._render_common(H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, code, kwargs)

    def render_fitting(self, H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, shapeCodes=None, uvCodes=None,
                       expType=20, expCodes=None, near=0., far=1., use_viewdirs=False, c2w_staticcam=None,
                       network_query_fn=None, **kwargs):
        """Fitting / novel-view entry: texture code given directly, expression code stored at slot 20
        (render_class.py:354-437)."""
        for k in ("network_fine", "network_fn"):            # (the reference crashes on network_fine=None; tolerated here)
            if kwargs.get(k) is not None:
                unwrap(kwargs[k]).eval()
        self.shapeCodes = shapeCodes
        self.expType = int(expType)
        self._weight_grads = bool(self.fit_weight_grads)
        if len(self.expCodes_Sigma) == 20:
            self.expCodes_Sigma.append(expCodes)
        else:
            self.expCodes_Sigma[20] = expCodes
        return self._render_common(H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, uvCodes,
                                   kwargs)

    def render_path(self, render_poses, hwf, K, chunk, render_kwargs, uvMap=None, expType=None, gt_imgs=None,
                    savedir=None, render_factor=0, shapeCodes=None, name=None):
        """Render one image per pose (render_class.py:199-237).  Existing outputs are skipped so a bulk render can
        resume.  Images are written as PNG when ``savedir`` is given and an encoder is importable."""
        height, width, focal = hwf
        if render_factor:                                   # render downsampled
            height, width, focal = height // render_factor, width // render_factor, focal / render_factor

        def out_file(i):
            stem = name if name is not None else "{:03d}".format(i)
            return os.path.join(savedir, stem + ".png")

        if savedir is not None and os.path.exists(os.path.join(savedir, "{}.png".format(name))):
            print("exists")                                 # bulk renders resume by skipping finished images
            return 0, 0
        from .io import PngSink
        frames, disparities = [], []
        shared = self.png_sink                              # a bulk driver may install one sink for the whole job, so that
        sink = shared if shared is not None else PngSink()  # encoding overlaps the NEXT render_path call as well
        try:                                                # quantise on device, pinned D2H, encode on worker threads
            for i, pose in enumerate(render_poses):
                rgb, disp, _acc, _extras = self.render(height, width, K, chunk=chunk, c2w=pose[:3, :4],
                                                       shapeCodes=shapeCodes[i, :].reshape(1, -1), uvMap=uvMap[i, :],
                                                       expType=expType[i], **render_kwargs)
                if savedir is not None:
                    # the verdict of THIS frame's launches travels with the frame: a snapshot + event of its own, taken here (after the
                    # frame's launches, before its copy), which the worker waits for before it writes the file (the shared
                    # mirror's event usually belonged to a LATER frame by the time the worker looked)
                    sink.submit(out_file(i), rgb, check=self.frame_check())
                frames.append(rgb.detach())
                disparities.append(disp.detach())
        finally:
            if shared is None:
                sink.close()
        out = torch.stack(frames, 0).cpu().numpy(), torch.stack(disparities, 0).cpu().numpy()
        self.check_launches(block=True)                     # (the copies above already waited for the device)
        return out

    # ------------------------------------------------------------------------------------------------
    def _set_codes(self, shapeCodes, expType, expCodes):
        """The conditioning of a geometry query, stored on ``self`` as ``render_fitting`` stores it: the shape code, the expression slot
        and — when given — the expression code at slot 20 (render_class.py:354-437)."""
        if shapeCodes is None:
            raise lib.MofaError("shapeCodes is required")
        self.shapeCodes = shapeCodes
        self.expType = int(expType)
        if expCodes is not None:
            if len(self.expCodes_Sigma) == 20:
                self.expCodes_Sigma.append(expCodes)
            else:
                self.expCodes_Sigma[20] = expCodes

    def _fold_density(self, network, dev):
        """The folded codes of a density query.  The texture code feeds only the uv layers, which a density query does not run: zeros
        fold as well as any code."""
        return self._fold_codes(network, torch.zeros(self._hip(network).ch_tex, dtype=torch.float32, device=dev)).clone()

    def _density_setup(self, what, network, shapeCodes, expType, expCodes, netchunk):
        """What ``query_density`` and ``extract_mesh``'s narrow band (``what``: the name in the error texts) do before their first launch:
        the chunk, the codes on ``self``, the network's device, the folded codes -> ``(HipNet, device, chunk, folded)``."""
        chunk = int(netchunk if netchunk is not None else self.netchunk)
        if chunk < 1:
            raise lib.MofaError(f"{what}: netchunk = {chunk}")
        self._set_codes(shapeCodes, expType, expCodes)
        h = self._hip(network)
        dev = next(unwrap(network).parameters()).device
        if dev.type != "cuda":
            raise lib.MofaError(f"{what}: the network must live on the GPU (net.cuda()); there is no CPU path")
        with torch.no_grad():
            return h, dev, chunk, self._fold_density(network, dev)

    def query_density(self, network, pts=None, *, bounds=None, resolution=None, shapeCodes, expType=20, expCodes=None, netchunk=None):
        """The network's density — the pre-ReLU ``raw[..., 3]`` of ``run_network``, bit for bit — at explicit points ``pts [N,3]``
        (returns ``[N]``) or on the grid ``bounds = ((x0,y0,z0), (x1,y1,z1))`` x ``resolution = (nx,ny,nz)`` (returns ``[nx,ny,nz]``, sample
        (i,j,k) at lo + (i,j,k) * step, step = (hi - lo) / (n - 1) in float32).  Density depends on the point, the shape code and the
        expression code only (models/model.py:121-128), so the texture branch, the view layer and the rgb head are not run
        (``mofa_net_density``).  Works in chunks of ``netchunk`` points (default ``self.netchunk``); the result does not depend on the
        chunk size.  Inference only: no autograd graph whatever ``torch.is_grad_enabled()`` says.  Waits for the launch verdicts
        (``check_launches(block=True)``) before it returns."""
        from . import mesh
        if (pts is None) == (bounds is None or resolution is None):
            raise lib.MofaError("query_density: give pts, or bounds and resolution")
        h, dev, chunk, folded = self._density_setup("query_density", network, shapeCodes, expType, expCodes, netchunk)
        with torch.no_grad():
            if pts is not None:
                if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[-1] != 3:
                    raise lib.MofaError(f"query_density: pts must be a [N,3] tensor, got {getattr(pts, 'shape', type(pts))}")
                if not pts.is_cuda:
                    raise lib.MofaError("query_density: pts is a CPU tensor; there is no CPU path")
                p = pts.detach().float().contiguous()
                out = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
                for i in range(0, p.shape[0], chunk):
                    h.density_points(p[i:i + chunk], out[i:i + chunk], folded)
            else:
                res, lo, step = mesh.grid_spec(bounds, resolution)
                n = res[0] * res[1] * res[2]
                out = torch.empty(n, dtype=torch.float32, device=dev)
                buf = torch.empty(min(chunk, n), 3, dtype=torch.float32, device=dev)
                for i in range(0, n, chunk):
                    m = min(chunk, n - i)
                    mesh.grid_points(res, lo, step, i, m, buf[:m])
                    h.density_points(buf[:m], out[i:i + m], folded)
                out = out.reshape(res)
        self.check_launches(block=True)
        return out

    _GEOMETRY_READS = ("network_fn", "network_fine", "N_samples", "N_importance", "perturb", "lindisp", "pytest", "raw_noise_std")
    _GEOMETRY_IGNORES = ("white_bkgd", "use_viewdirs", "retraw", "network_query_fn", "verbose")     # none of them changes geometry

    def render_geometry(self, H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., shapeCodes=None, expType=20,
                        expCodes=None, c2w_staticcam=None, occupancy=None, retweights=False, median=False, points=False, normals=False,
                        surface="median", acc_min=0.5, median_threshold=0.5, **render_kwargs):
        """Geometry-only render: ``depth, disp, acc, extras`` of a frame from the density alone — no texture stack, no view layer, no rgb
        head, one float per sample instead of four.  Takes the ``render_kwargs_test`` dictionary the scripts hand to
        :meth:`render_fitting` (``network_fn``, ``network_fine``, ``N_samples``, ``N_importance``, ``perturb``, ``lindisp``, ``pytest``
        are read; ``white_bkgd``, ``use_viewdirs``, ``retraw``, ``network_query_fn`` and ``verbose`` change no geometry and are
        ignored; ``raw_noise_std > 0`` and unknown keys are refused).  There is no texture argument: the texture code never reaches the
        density (models/model.py:121-128).

        Everything geometric in a frame depends on density alone (render_class.py:440-482), so ``disp``, ``acc``, the coarse ``disp0`` /
        ``acc0`` and ``z_std`` are the bits :meth:`render_fitting` returns for the same rays and codes, and ``depth`` / ``weights`` the bits
        ``mofa_composite_forward`` computes inside it and drops.  Per pass: ``mofa_ray_points`` on sub-batches of ``netchunk`` points,
        ``HipNet.density_points``, ``mofa_composite_sigma``; between the passes ``mofa_sample_pdf_merge`` as in :meth:`render_rays`.
        ``occupancy`` (an ``occupancy.OccupancyGrid``): the density runs on the kept samples only, as in the culled :meth:`render_rays`
        (``self.occupancy_stats`` is filled the same way).  ``extras``: ``depth0``, ``disp0``, ``acc0``, ``z_std`` when a fine pass ran;
        with ``retweights=True`` also ``weights`` and ``z_vals`` of the final pass.  Inference only: runs under ``torch.no_grad()`` on
        detached inputs.  No host synchronisation apart from the culled passes' kept counts; ``frame_check`` / ``check_launches`` work
        afterwards as for :meth:`render`.

        Surface buffers (all off by default; with all of them off the method launches exactly what it launches without them), formed
        on the final pass — the fine one if it ran, otherwise the coarse one — and returned in ``extras``:

        * ``median=True``: ``depth_median`` and ``median_index`` (int32) from ``mofa_depth_median`` on the pass's compositing weights,
          per chunk of rays: the first sample whose accumulated weight reaches ``median_threshold``; rays on which it never does get
          index -1 and the last sample's depth.
        * ``points=True``: ``points [...,3] = o + d * depth_surface`` (``mofa_ray_points``, one sample per ray), where
          ``depth_surface`` is ``depth_median`` for ``surface="median"`` and the expected depth ``depth`` for ``surface="expected"``.
        * ``normals=True``: ``normals [H,W,3]`` and ``normals_valid [H,W]`` (uint8) from ``mofa_point_normals`` on the whole frame's
          points, ``acc`` and ray directions: screen-space differences between pixels with ``acc >= acc_min``, facing the camera,
          zero where invalid.  Needs a 2-D grid of rays: ``c2w``, or ``rays`` shaped ``[2,H,W,3]``.

        ``normals`` implies ``points``, and ``points`` with ``surface="median"`` implies ``median``; what was implied is returned as
        well.  ``points`` and ``normals`` are refused with ``ndc=True``: the sampler's rays are NDC rays then, and neither a point on
        them nor a difference of such points is a position or a direction in the scene."""
        if surface not in ("median", "expected"):
            raise lib.MofaError(f"render_geometry: surface = {surface!r} (want 'median' or 'expected')")
        if not (np.isfinite(_scalar(median_threshold)) and _scalar(median_threshold) > 0.):
            raise lib.MofaError(f"render_geometry: median_threshold = {_scalar(median_threshold)} (want a finite value > 0)")
        if not np.isfinite(_scalar(acc_min)):
            raise lib.MofaError(f"render_geometry: acc_min = {_scalar(acc_min)} (want a finite value)")
        want_points = bool(points or normals)
        want_median = bool(median or (want_points and surface == "median"))
        if normals and c2w is None and (rays is None or rays[1].dim() != 3):
            raise lib.MofaError("render_geometry: normals=True needs a 2-D grid of rays (c2w, or rays shaped [2,H,W,3]); got a flat list of rays "
                                f"{[2] + list(rays[1].shape) if rays is not None else None}")
        if want_points and ndc:
            raise lib.MofaError("render_geometry: points / normals with ndc=True: the sampler's rays are NDC rays, a point on them is no scene "
                                "position (render with ndc=False)")
        for k in render_kwargs:
            if k not in self._GEOMETRY_READS and k not in self._GEOMETRY_IGNORES:
                raise lib.MofaError(f"render_geometry: unknown argument {k!r} (reads {', '.join(self._GEOMETRY_READS)}; ignores "
                                    f"{', '.join(self._GEOMETRY_IGNORES)})")
        noise_std = render_kwargs.get("raw_noise_std", 0.)
        if noise_std is not None and _scalar(noise_std) > 0.:
            raise lib.MofaError(f"render_geometry: raw_noise_std = {_scalar(noise_std)}: density noise is a training regulariser; the "
                                "geometry render is for inference (raw_noise_std = 0)")
        if render_kwargs.get("network_fn") is None or render_kwargs.get("N_samples") is None:
            raise lib.MofaError("render_geometry: network_fn and N_samples are required (pass the render_kwargs_test dictionary)")
        network_fn, network_fine = render_kwargs["network_fn"], render_kwargs.get("network_fine")
        S, Ni = int(render_kwargs["N_samples"]), int(render_kwargs.get("N_importance", 0) or 0)
        perturb, lindisp, pytest = render_kwargs.get("perturb", 0.), bool(render_kwargs.get("lindisp", False)), bool(render_kwargs.get("pytest", False))
        L = self._lib()
        with torch.no_grad():
            rays_o, rays_d, viewdirs, sh = self._make_rays(H, W, K, c2w, rays, True, c2w_staticcam, ndc)
            if c2w is None and not (rays[0].is_cuda and rays[1].is_cuda):
                raise lib.MofaError("render_geometry: the rays are CPU tensors; there is no CPU path")
            rays_o, rays_d, viewdirs = (t.detach().float().contiguous() for t in (rays_o, rays_d, viewdirs))
            dev, n_rays = rays_o.device, int(rays_o.shape[0])
            near, far = self._bounds(near, far, rays_d)
            self._set_codes(shapeCodes, expType, expCodes)
            self.occupancy_stats = None
            if occupancy is not None:
                self._check_occupancy(occupancy, rays_o, 0., network_fn, network_fine)
                self.occupancy_stats = {}
            fine_pass = Ni > 0 and self.is_run_fineNet
            fine = network_fn if network_fine is None else network_fine
            nets = [network_fn] + ([fine] if fine_pass and fine is not network_fn else [])
            folded = {id(n): self._fold_density(n, dev) for n in nets}
            st = lib.stream()
            out: Dict[str, list] = {}
            for b0 in range(0, n_rays, int(chunk)):
                ro, rd, vd = rays_o[b0:b0 + chunk], rays_d[b0:b0 + chunk], viewdirs[b0:b0 + chunk]
                R = int(ro.shape[0])
                bounds = (near[b0:b0 + chunk], far[b0:b0 + chunk]) if torch.is_tensor(near) else (near, far)
                z, z_stride = self._coarse_positions(*bounds, R, S, lindisp, perturb, pytest, dev)

                def one_pass(net, zv, zs, n_s, which):
                    h, fold = self._hip(net), folded[id(net)]
                    sigma = torch.empty(R, n_s, dtype=torch.float32, device=dev)
                    if occupancy is None:
                        rays_per = max(1, int(self.netchunk) // n_s)
                        pts = torch.empty(min(R, rays_per) * n_s, 3, dtype=torch.float32, device=dev)
                        for i in range(0, R, rays_per):
                            j = min(R, i + rays_per)
                            m = (j - i) * n_s
                            lib.check(L.mofa_ray_points(lib.ptr(ro[i:j]), lib.ptr(rd[i:j]), lib.ptr(zv[i:j] if zs else zv), zs, j - i, n_s,
                                                        lib.ptr(pts[:m]), st), "mofa_ray_points")
                            h.density_points(pts[:m], sigma[i:j].reshape(-1), fold)
                    else:      # classify, compact (one host read: n_kept), density of the kept points, scatter (writes every element)
                        cp = self._culled_pass(occupancy, which, ro, rd, zv, zs, n_s)
                        kept = None
                        if cp.n_kept:
                            pts, _, _ = cp.gather(vd)
                            kept = torch.empty(cp.n_kept, dtype=torch.float32, device=dev)
                            per = max(1, int(self.netchunk))
                            for i in range(0, cp.n_kept, per):
                                h.density_points(pts[i:i + per], kept[i:i + per], fold)
                        cp.scatter_sigma(kept, sigma)
                    o = {k: torch.empty(R, *shp, dtype=torch.float32, device=dev)
                         for k, shp in (("disp", ()), ("acc", ()), ("depth", ()), ("weights", (n_s,)))}
                    lib.check(L.mofa_composite_sigma(lib.ptr(sigma), lib.ptr(zv), zs, lib.ptr(rd), None, R, n_s, lib.ptr(o["disp"]),
                                                     lib.ptr(o["acc"]), lib.ptr(o["depth"]), lib.ptr(o["weights"]), st), "mofa_composite_sigma")
                    return o

                c = one_pass(network_fn, z, z_stride, S, "coarse")
                ret = {"depth": c["depth"], "disp": c["disp"], "acc": c["acc"]}
                z_last, w_last = (z if z_stride else z[None, :].expand(R, S)), c["weights"]
                z_med, zs_med = z, z_stride
                if fine_pass:
                    _, z_fine, z_std = self._importance_positions(z, z_stride, c["weights"], R, S, Ni, perturb, pytest, dev)
                    f = one_pass(fine, z_fine, S + Ni, S + Ni, "fine")
                    ret = {"depth": f["depth"], "disp": f["disp"], "acc": f["acc"], "depth0": c["depth"], "disp0": c["disp"],
                           "acc0": c["acc"], "z_std": z_std}
                    z_last, w_last = z_fine, f["weights"]
                    z_med, zs_med = z_fine, S + Ni
                if retweights:
                    ret["weights"], ret["z_vals"] = w_last, z_last
                if want_median:      # on the final pass's compositing weights, as the kernel wrote them
                    ret["depth_median"] = torch.empty(R, dtype=torch.float32, device=dev)
                    ret["median_index"] = torch.empty(R, dtype=torch.int32, device=dev)
                    lib.check(L.mofa_depth_median(lib.ptr(w_last), lib.ptr(z_med), zs_med, R, int(w_last.shape[1]), _scalar(median_threshold),
                                                  lib.ptr(ret["depth_median"]), ret["median_index"].data_ptr(), st), "mofa_depth_median")
                for k, v in ret.items():
                    out.setdefault(k, []).append(v)
            full = {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in out.items()}
            if want_points:          # one launch each on the whole frame: a normal reads its pixel's neighbours, which a chunk of rays cuts apart
                surf = (full["depth_median"] if surface == "median" else full["depth"]).contiguous()
                full["points"] = torch.empty(n_rays, 3, dtype=torch.float32, device=dev)
                lib.check(L.mofa_ray_points(lib.ptr(rays_o), lib.ptr(rays_d), lib.ptr(surf), 1, n_rays, 1, lib.ptr(full["points"]), st),
                          "mofa_ray_points")
            if normals:
                full["normals"] = torch.empty(n_rays, 3, dtype=torch.float32, device=dev)
                full["normals_valid"] = torch.empty(n_rays, dtype=torch.uint8, device=dev)
                lib.check(L.mofa_point_normals(lib.ptr(full["points"]), lib.ptr(full["acc"].contiguous()), lib.ptr(rays_d), int(sh[0]), int(sh[1]),
                                               _scalar(acc_min), lib.ptr(full["normals"]), full["normals_valid"].data_ptr(), st),
                          "mofa_point_normals")
            full = {k: torch.reshape(v, list(sh[:-1]) + list(v.shape[1:])) for k, v in full.items()}
        return [full.pop("depth"), full.pop("disp"), full.pop("acc"), full]

    _PATH_GEOMETRY_OPTIONS = ("surface", "acc_min", "median_threshold", "occupancy")

    def render_path_geometry(self, render_poses, hwf, K, chunk, render_kwargs, expType=None, expCodes=None, shapeCodes=None, savedir=None,
                             render_factor=0, name=None, near=None, far=None, **surface):
        """The geometry twin of :meth:`render_path`: one :meth:`render_geometry` frame per pose with its surface buffers on (normals,
        points and — for ``surface="median"`` — the median depth).  ``surface`` options: ``surface``, ``acc_min``, ``median_threshold``,
        ``occupancy``.  ``near`` / ``far`` (scalars) default to the ones in ``render_kwargs``, ``ndc`` to ``render_kwargs["ndc"]`` and, without one, to
        ``False`` (points and normals are refused on NDC rays).  ``shapeCodes`` / ``expCodes`` with one row
        per pose are taken row by row, otherwise shared; ``expType`` likewise (default 20).

        With ``savedir`` three 8-bit PNGs per pose go through the ``PngSink`` with the frame's ``frame_check``: ``<stem>_normals.png``
        (``valid * (n + 1) / 2``: invalid pixels are black), ``<stem>_mask.png`` (the pixels with ``acc >= acc_min``) and
        ``<stem>_depth.png`` (``(depth_surface - near) / (far - near)`` in grey); ``stem`` is the pose's number, or ``name`` (followed by
        the number when there are several poses).  A pose whose three files exist is skipped, so a bulk render can resume.  Returns a
        dict of numpy arrays stacked over the rendered poses — ``depth``, ``disp``, ``acc``, ``depth_surface``, ``points``, ``normals``,
        ``normals_valid`` and ``depth_median`` / ``median_index`` when they were formed — with ``rendered`` and ``skipped``, the lists
        of pose numbers."""
        for k in surface:
            if k not in self._PATH_GEOMETRY_OPTIONS:
                raise lib.MofaError(f"render_path_geometry: unknown argument {k!r} (surface options: {', '.join(self._PATH_GEOMETRY_OPTIONS)})")
        height, width, focal = hwf
        if render_factor:                                   # render downsampled
            height, width, focal = height // render_factor, width // render_factor, focal / render_factor
        kw = dict(render_kwargs)
        kw_near, kw_far = kw.pop("near", None), kw.pop("far", None)
        ndc = kw.pop("ndc", False)
        near, far = (kw_near if near is None else near), (kw_far if far is None else far)
        if near is None or far is None:
            raise lib.MofaError("render_path_geometry: near and far are required (as arguments or in render_kwargs)")
        near, far = _scalar(near), _scalar(far)
        if not far > near:
            raise lib.MofaError(f"render_path_geometry: near = {near}, far = {far} (want far > near)")
        n_poses = len(render_poses)
        which = surface.get("surface", "median")
        acc_min = surface.get("acc_min", 0.5)

        def row(v, i):
            return v[i].reshape(1, -1) if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == n_poses and n_poses > 1 else v

        def frame(i, paths, sink):
            et = 20 if expType is None else (expType[i] if hasattr(expType, "__len__") else expType)
            depth, disp, acc, ex = self.render_geometry(height, width, K, chunk=chunk, c2w=render_poses[i][:3, :4], ndc=ndc, near=near, far=far,
                                                        shapeCodes=row(shapeCodes, i), expType=et, expCodes=row(expCodes, i),
                                                        normals=True, **surface, **kw)
            surf = ex["depth_median"] if which == "median" else depth
            if paths is not None:
                valid = ex["normals_valid"].to(torch.float32)[..., None]
                grey = lambda t: t[..., None].expand(*t.shape, 3)
                span = torch.full_like(surf, far - near)          # a tensor divisor: an elementwise, correctly rounded division
                check = self.frame_check()                       # one snapshot of this frame's verdicts for its three files
                for f, img in zip(paths, (valid * ((ex["normals"] + 1.) / 2.), grey((acc >= _scalar(acc_min)).to(torch.float32)),
                                          grey((surf - near) / span))):
                    sink.submit(f, img, check=check)
            return dict(ex, depth=depth, disp=disp, acc=acc, depth_surface=surf)

        out = self._pose_loop(n_poses, name, savedir, ("_normals.png", "_mask.png", "_depth.png"), frame)
        self.check_launches(block=True)
        return out

    def _pose_loop(self, n_poses, name, savedir, tails, frame):
        """The loop of :meth:`render_path_geometry` and :meth:`render_path_mesh`: for each pose number ``i``, ``frame(i, paths, sink)``
        -> a dict of tensors, where ``paths`` are the pose's files ``<savedir>/<stem><tail>`` (``None`` without ``savedir``; ``stem`` is the
        pose's number, or ``name``, followed by the number when there are several poses) and ``sink`` the ``PngSink`` to submit them to
        (``self.png_sink``, or one of the loop's own, closed at its end).  A pose whose files all exist is skipped, so a bulk render can
        resume.  Returns the dicts stacked over the rendered poses as numpy arrays, with ``rendered`` and ``skipped``, the lists of pose
        numbers."""
        def stem(i):
            if name is None:
                return "{:03d}".format(i)
            return str(name) if n_poses == 1 else "{}_{:03d}".format(name, i)

        from .io import PngSink
        frames: Dict[str, list] = {}
        rendered, skipped = [], []
        shared = self.png_sink
        sink = shared if shared is not None else PngSink()
        try:
            for i in range(n_poses):
                paths = [os.path.join(savedir, stem(i) + tail) for tail in tails] if savedir is not None else None
                if paths is not None and all(os.path.exists(f) for f in paths):
                    skipped.append(i)
                    continue
                tensors = frame(i, paths, sink)
                rendered.append(i)
                for k, v in tensors.items():
                    frames.setdefault(k, []).append(v.detach())
        finally:
            if shared is None:
                sink.close()
        out = {k: torch.stack(v, 0).cpu().numpy() for k, v in frames.items()}
        out["rendered"], out["skipped"] = rendered, skipped
        return out

    def render_mesh(self, H, W, K, c2w, verts, faces, colors=None, znear=1e-3, ambient=0.3, texture=None, uvs=None, uv_faces=None):
        """A view of a triangle mesh — what :meth:`extract_mesh` returns — from the camera ``K`` / ``c2w`` of ``get_rays``, by the GPU
        rasteriser (``mesh.rasterize``; no network runs).  Returns ``(rgb [H,W,3], depth [H,W], mask [H,W] bool, extras)``; ``depth`` is
        the ray parameter of the pixel's ray, the depth :meth:`render_geometry` gives without NDC, and 0 where nothing is hit.  With
        ``colors [V,3]`` (``extract_mesh(colors=True)``) ``rgb`` is the perspective-correct interpolation of the vertex colours; without,
        a head-light shade of the flat face normal ``n`` (turned to the camera): ``ambient + (1 - ambient) max(0, -n . d / |d|)`` for
        the pixel's ray direction ``d``, black where nothing is hit.  ``extras``: ``face`` (int32, -1 where nothing is hit), ``counts``
        (device int64 [4]: faces drawn, culled, degenerate, on the wavefront path) and, for the shade, ``normal``.

        With ``texture [Ht,Wt,3]`` and the mesh's UV layout ``uvs [T,2]`` / ``uv_faces [F,3]`` (:meth:`bake_texture`, ``mesh.texel_map``)
        ``rgb`` is ``mesh.sample_texture`` of the rasterised ``face`` / ``bary`` — a bilinear lookup per pixel, black where nothing is
        hit — and ``extras`` holds ``bary`` too; like ``colors``, a texture is shown as it is: ``ambient`` belongs to the shade alone and
        is not read.  ``colors`` together with ``texture`` is refused.  Without the three arguments nothing changes."""
        from . import mesh
        from .rays import get_rays
        if texture is not None or uvs is not None or uv_faces is not None:
            if colors is not None:
                raise lib.MofaError("render_mesh: colors and texture are two ways to colour the mesh: give one")
            if texture is None or uvs is None or uv_faces is None:
                raise lib.MofaError("render_mesh: texture, uvs and uv_faces go together")
            if not torch.is_tensor(texture) or texture.dim() != 3 or texture.shape[-1] != 3:
                raise lib.MofaError(f"render_mesh: want texture [Ht,Wt,3], got {tuple(texture.shape) if torch.is_tensor(texture) else type(texture).__name__}")
            _, F, _ = mesh._mesh_tensors("render_mesh", verts, faces)
            if not torch.is_tensor(uv_faces) or uv_faces.dim() != 2 or uv_faces.shape[0] != F:
                raise lib.MofaError(f"render_mesh: uv_faces {tuple(uv_faces.shape) if torch.is_tensor(uv_faces) else type(uv_faces).__name__} for "
                                    f"{F} faces (want one row of UV indices per face)")
            out = mesh.rasterize(verts, faces, H, W, K, c2w, znear=znear, bary=True)
            rgb = mesh.sample_texture(texture, out["face"], out["bary"], uvs, uv_faces, background=0.0)
            return rgb, out["depth"], out["mask"], {"face": out["face"], "counts": out["counts"], "bary": out["bary"]}
        if colors is not None:
            if colors.dim() != 2 or colors.shape[-1] != 3:
                raise lib.MofaError(f"render_mesh: want colors [V,3], got {tuple(colors.shape)}")
            out = mesh.rasterize(verts, faces, H, W, K, c2w, attrs=colors, znear=znear)
            rgb = out["attr"]
            extras = {"face": out["face"], "counts": out["counts"]}
        else:
            ambient = _scalar(ambient)
            if not 0. <= ambient <= 1.:
                raise lib.MofaError(f"render_mesh: ambient = {ambient} (want 0 .. 1)")
            out = mesh.rasterize(verts, faces, H, W, K, c2w, znear=znear, normals=True)
            _, d = get_rays(H, W, K, c2w, device=verts.device)
            view = d / d.norm(dim=-1, keepdim=True)
            shade = ambient + (1. - ambient) * (-(out["normal"] * view).sum(-1)).clamp(min=0.)
            rgb = (shade * out["mask"].to(torch.float32))[..., None].expand(H, W, 3).contiguous()
            extras = {"face": out["face"], "counts": out["counts"], "normal": out["normal"]}
        return rgb, out["depth"], out["mask"], extras

    def mesh_bounds(self, H, W, K, c2w, verts, faces, near, far, margin, ndc=False, grid=None):
        """Per-ray sampling bounds that hug a mesh of the face — what :meth:`extract_mesh` returns, possibly filtered, simplified or
        smoothed — for the camera ``K`` / ``c2w``: the rays :meth:`render_fitting` itself generates for that pose are cast against the
        mesh (``mesh.ray_bounds``: first and last hit in ``[near, far]``, widened by ``margin``, clipped to ``[near, far]``; no network
        runs).  Returns ``(near [H*W,1], far [H*W,1], hit [H,W] bool)``: ``render_fitting(..., near=n, far=f, ndc=False)`` and
        :meth:`render_geometry` take the two columns as they are, and ``hit`` is the silhouette before any sample is drawn.  A ray that
        misses the mesh keeps the scalar bounds.  ``ndc=True`` is refused: the sampler's rays are NDC rays then, and the mesh lives in
        scene space."""
        from . import mesh
        if ndc:
            raise lib.MofaError("mesh_bounds: ndc=True: the sampler's rays are NDC rays, the mesh lives in scene space (render with ndc=False)")
        if c2w is None:
            raise lib.MofaError("mesh_bounds: needs the camera pose c2w")
        rays_o, rays_d, _, _ = self._make_rays(H, W, K, c2w, None, True, None, False)
        b = mesh.ray_bounds(rays_o, rays_d, verts, faces, near, far, margin, grid=grid)
        return b["near"].reshape(-1, 1), b["far"].reshape(-1, 1), b["hit"].reshape(int(H), int(W))

    def fuse_geometry(self, render_poses, H, W, K, *, bounds, resolution, trunc, shapeCodes, expType=20, expCodes=None, surface="median",
                      acc_min=0.5, background="empty", weight=None, unobserved="auto", close_border=True, **render_kwargs):
        """A mesh of the face with NO density level: one :meth:`render_geometry` frame per pose of ``render_poses`` is fused into a
        truncated signed distance volume over ``bounds`` / ``resolution`` (``mesh.tsdf_volume`` / ``tsdf_integrate``, truncation ``trunc``
        in scene units) and the volume's zero level is marched (``mesh.tsdf_surface``) — the surface the renderer itself shows from
        those poses.  Returns ``(verts [V,3] float32, faces [F,3] int32, stats)``; the mesh is what :meth:`extract_mesh` returns in kind,
        so ``mesh.components``, ``simplify``, ``smooth``, ``surface_distance`` and the rest take it as it is.

        Per frame: the depth is ``depth_median`` (``surface="median"``) or the expected depth (``"expected"``), the mask
        ``acc >= acc_min``; ``mesh.depth_frame`` encodes the pixels outside the mask as empty space (``background="empty"``: their rays
        carve the volume) or as unknown (``"unknown"``), and the frame is integrated as soon as it is rendered — no list of frames is
        kept.  ``weight="acc"`` weighs a pixel's observation by ``acc`` inside the mask and by ``1 - acc`` outside it (clamped at 0);
        ``None`` weighs every pixel 1.  ``unobserved`` / ``close_border`` are ``mesh.tsdf_field``'s.  ``render_kwargs`` go to
        :meth:`render_geometry` (``near``, ``far``, ``occupancy``, ``chunk``, ``median_threshold`` and the ``render_kwargs_test``
        dictionary); ``ndc=True`` is refused as in :meth:`mesh_bounds`: the depth would be an NDC depth, the volume lives in scene space.

        ``stats``: the field's counters (``observed``, ``filled_inside``, ``filled_outside``, ``border``, ``voxels``, ``frames``),
        ``hit_share`` (per frame, the share of pixels inside the mask), ``trunc``, ``resolution`` and ``times`` (seconds spent rendering,
        integrating and marching, each phase waited for).  ``self.fuse_state`` keeps the volume.  Which ``trunc`` and ``acc_min`` suit a
        trained face has not been measured."""
        from . import mesh
        who = "fuse_geometry"
        if render_kwargs.pop("ndc", False):
            raise lib.MofaError(f"{who}: ndc=True: the rendered depth is an NDC depth, the volume lives in scene space (render with ndc=False)")
        if surface not in ("median", "expected"):
            raise lib.MofaError(f"{who}: surface = {surface!r} (want 'median' or 'expected')")
        if background not in ("empty", "unknown"):
            raise lib.MofaError(f"{who}: background = {background!r} (want 'empty' or 'unknown')")
        if weight not in (None, "acc"):
            raise lib.MofaError(f"{who}: weight = {weight!r} (want None or 'acc')")
        if unobserved not in ("auto", "outside", "inside"):
            raise lib.MofaError(f"{who}: unobserved = {unobserved!r} (want 'auto', 'outside' or 'inside')")
        if not np.isfinite(_scalar(acc_min)):
            raise lib.MofaError(f"{who}: acc_min = {_scalar(acc_min)} (want a finite value)")
        trunc = float(trunc)
        if not (np.isfinite(trunc) and trunc > 0):
            raise lib.MofaError(f"{who}: trunc = {trunc} (want finite and > 0)")
        res, lo, step = mesh.grid_spec(bounds, resolution)
        poses = [p for p in render_poses]
        if not poses:
            raise lib.MofaError(f"{who}: no poses")
        H, W = int(H), int(W)
        state, shares = None, []
        times = {"render": 0.0, "integrate": 0.0, "march": 0.0}
        with torch.no_grad():
            for pose in poses:
                t0 = time.perf_counter()
                depth, _, acc, extras = self.render_geometry(H, W, K, c2w=pose, ndc=False, shapeCodes=shapeCodes, expType=expType, expCodes=expCodes,
                                                             median=surface == "median", **render_kwargs)
                if surface == "median":
                    depth = extras["depth_median"]
                depth, acc = depth.reshape(H, W), acc.reshape(H, W)
                torch.cuda.synchronize(depth.device)
                t1 = time.perf_counter()
                if state is None:
                    state = mesh.tsdf_volume(res, lo, step, trunc, depth.device)
                mask = acc >= float(acc_min)
                frame = mesh.depth_frame(depth.contiguous(), mask, background)
                w = torch.clamp(torch.where(mask, acc, 1.0 - acc), min=0.0).contiguous() if weight == "acc" else None
                mesh.tsdf_integrate(state, frame, K, pose, weight=w, carve=True)
                shares.append(mask.float().mean())
                torch.cuda.synchronize(depth.device)
                t2 = time.perf_counter()
                times["render"] += t1 - t0
                times["integrate"] += t2 - t1
            t0 = time.perf_counter()
            field, stats = mesh.tsdf_field(state, unobserved, close_border)
            verts, faces = mesh.iso_surface(field, 0.0, lo, step)
            torch.cuda.synchronize(field.device)
            times["march"] = time.perf_counter() - t0
        stats.update(hit_share=[float(s) for s in torch.stack(shares).cpu()], trunc=trunc, resolution=res, times=times)
        self.fuse_state = state
        self.check_launches(block=True)
        return verts, faces, stats

    def bake_mesh(self, render_poses, H, W, K, verts, faces, *, depth_tol, shapeCodes, uvCodes, expCodes=None, expType=20, blend="mean",
                  cos_min=0.0, power=2, fill_iterations=0, chunk=1024 * 32, normals=None, **render_kwargs):
        """Vertex colours for a mesh with ANY triangulation — an extraction, or a template that was warped, simplified or smoothed off the
        level set — from the renderer's own frames: per pose of ``render_poses`` one :meth:`render_fitting` colour frame (``ndc=False``,
        compositing along every ray, texture code ``uvCodes``) is projected onto the vertices (``mesh.bake_integrate``) as soon as it is
        rendered; no list of frames is kept.  What a vertex may take from a view is decided by the mesh itself: its visibility depth is
        ``mesh.rasterize`` of ``verts`` / ``faces`` from that pose through ``mesh.depth_frame``, its normals are ``mesh.vertex_normals``
        (or ``normals [V,3]``, e.g. ``extract_mesh``'s density normals).
        Returns ``(colors [V,3] float32, valid [V] bool, stats)``; ``mesh.write_ply(colors=...)`` and :meth:`render_mesh` show them, and
        colours of meshes in one vertex numbering stack into ``mesh.shape_model``.

        ``depth_tol`` (scene units) is required: no value has been measured for a trained face.  ``blend``, ``cos_min`` and ``power`` are
        ``mesh.bake_colors``' and ``mesh.bake_integrate``'s (untuned defaults); ``fill_iterations > 0`` closes the holes with
        ``mesh.fill_colors``.  ``render_kwargs`` go to :meth:`render_fitting` (``near``, ``far``, ``occupancy`` and the
        ``render_kwargs_test`` dictionary); ``ndc=True`` is refused as in :meth:`fuse_geometry`: the mesh lives in scene space.

        ``stats``: ``mesh.bake_colors``' counts (``colored``, ``occluded``, ``grazing``, ``unseen``, ``vertices``, ``frames``) as they
        stood BEFORE any filling, ``remaining`` (the vertices still invalid at the end), ``hit_share`` (per frame, the share of pixels the
        mesh covers) and ``times`` (seconds spent rendering, rasterising, integrating and resolving, each phase waited for).
        ``self.bake_stats`` keeps them, ``self.bake_state`` the state."""
        from . import mesh
        who = "bake_mesh"
        if render_kwargs.pop("ndc", False):
            raise lib.MofaError(f"{who}: ndc=True: the frames would be rendered in NDC space, the mesh lives in scene space (render with ndc=False)")
        if blend not in ("mean", "best"):
            raise lib.MofaError(f"{who}: blend = {blend!r} (want 'mean' or 'best')")
        depth_tol, cos_min, power = mesh._bake_params(who, depth_tol, cos_min, power)
        if isinstance(fill_iterations, bool) or not isinstance(fill_iterations, (int, np.integer)) or not 0 <= int(fill_iterations) <= mesh.BAKE_MAX_FILL:
            raise lib.MofaError(f"{who}: fill_iterations = {fill_iterations!r} (want an integer 0 .. {mesh.BAKE_MAX_FILL})")
        V, F, dev = mesh._mesh_tensors(who, verts, faces)
        poses = [p for p in render_poses]
        if not poses:
            raise lib.MofaError(f"{who}: no poses")
        H, W = int(H), int(W)
        times = {"render": 0.0, "rasterize": 0.0, "integrate": 0.0, "resolve": 0.0}
        shares = []
        with torch.no_grad():
            if normals is None:
                normals = mesh.vertex_normals(verts, faces).contiguous()
            state = mesh.bake_state(V, 3, dev)
            for pose in poses:
                t0 = time.perf_counter()
                rgb = self.render_fitting(H, W, K, chunk=chunk, c2w=pose, ndc=False, shapeCodes=shapeCodes, uvCodes=uvCodes, expType=expType,
                                          expCodes=expCodes, **render_kwargs)[0]
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                r = mesh.rasterize(verts, faces, H, W, K, pose)
                frame = mesh.depth_frame(r["depth"], r["mask"], "empty")
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                mesh.bake_integrate(state, verts, rgb.reshape(H, W, 3).contiguous(), frame, K, pose, normals, depth_tol=depth_tol, cos_min=cos_min,
                                    power=power)
                shares.append(r["mask"].float().mean())
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
                times["render"] += t1 - t0
                times["rasterize"] += t2 - t1
                times["integrate"] += t3 - t2
            t0 = time.perf_counter()
            baked = mesh.bake_colors(state, blend)
            colors, valid, stats = baked["colors"], baked["valid"], dict(baked["counts"])
            remaining = stats["vertices"] - stats["colored"]
            if fill_iterations:
                colors, valid, remaining = mesh.fill_colors(colors, valid, faces, int(fill_iterations))
            torch.cuda.synchronize(dev)
            times["resolve"] = time.perf_counter() - t0
        stats.update(remaining=int(remaining), hit_share=[float(s) for s in torch.stack(shares).cpu()], times=times, blend=blend,
                     depth_tol=depth_tol, cos_min=cos_min, power=power)
        self.bake_state, self.bake_stats = state, stats
        self.check_launches(block=True)
        return colors, valid, stats

    def bake_texture(self, render_poses, H, W, K, verts, faces, uvs, uv_faces, *, size=512, depth_tol, shapeCodes, uvCodes, expCodes=None,
                     expType=20, blend="mean", cos_min=0.0, power=2, dilate=8, normals=None, chunk=1024 * 32, **render_kwargs):
        """A texture image for a mesh with a UV layout (``uvs [T,2]`` float32, ``uv_faces [F,3]`` int32, per corner as in an OBJ; a
        template's own, or ``mesh.face_atlas`` for a mesh without one) from the renderer's own frames: :meth:`bake_mesh`'s loop with the
        surface points of the texels in place of the vertices.  ``mesh.texel_map`` finds the face and barycentrics of every texel centre
        of a ``size`` (an int or ``(Ht, Wt)``) image once, ``mesh.texel_surface`` makes their points and normals (the interpolation of
        ``normals [V,3]``, default ``mesh.vertex_normals``); then per pose one :meth:`render_fitting` colour frame (``ndc=False``) is
        projected onto them by ``mesh.bake_integrate`` against ``mesh.rasterize``'s depth of the mesh itself.  ``mesh.texture_image``
        resolves (``blend``), scatters and fills the gutters (``dilate`` steps).
        Returns ``(texture [Ht,Wt,3] float32, valid [Ht,Wt] bool, stats)``.  With ``size=512`` the texture is the tensor
        ``render(uvMap=...)`` takes; ``mesh.write_obj(texture=...)`` writes OBJ + MTL + PNG, and :meth:`render_mesh` shows it.

        ``depth_tol`` is required and ``blend``, ``cos_min``, ``power`` are untuned, as in :meth:`bake_mesh`; ``ndc=True`` is refused.
        ``stats``: :meth:`bake_mesh`'s keys — the counts are over the covered texels (``vertices`` = their number), taken before dilation;
        ``remaining`` the texels invalid at the end — plus the map's ``covered``, ``multi``, ``degenerate``, ``faces_without_texels``,
        ``size``, and ``times["texel_map"]`` (the map and the surface points).  ``self.bake_stats`` / ``self.bake_state`` keep stats and
        state, ``self.bake_map`` the texel map."""
        from . import mesh
        who = "bake_texture"
        if render_kwargs.pop("ndc", False):
            raise lib.MofaError(f"{who}: ndc=True: the frames would be rendered in NDC space, the mesh lives in scene space (render with ndc=False)")
        if blend not in ("mean", "best"):
            raise lib.MofaError(f"{who}: blend = {blend!r} (want 'mean' or 'best')")
        depth_tol, cos_min, power = mesh._bake_params(who, depth_tol, cos_min, power)
        if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or not 0 <= int(dilate) <= mesh.BAKE_MAX_FILL:
            raise lib.MofaError(f"{who}: dilate = {dilate!r} (want an integer 0 .. {mesh.BAKE_MAX_FILL})")
        V, F, dev = mesh._mesh_tensors(who, verts, faces)
        T, Fu, udev = mesh._uv_layout(who, uvs, uv_faces)
        if Fu != F or udev != dev:
            raise lib.MofaError(f"{who}: {Fu} UV faces on {udev} for {F} faces on {dev} (want one row of UV indices per face, on one device)")
        size = mesh._texture_size(who, size)
        poses = [p for p in render_poses]
        if not poses:
            raise lib.MofaError(f"{who}: no poses")
        H, W = int(H), int(W)
        times = {"texel_map": 0.0, "render": 0.0, "rasterize": 0.0, "integrate": 0.0, "resolve": 0.0}
        shares = []
        with torch.no_grad():
            t0 = time.perf_counter()
            if normals is None:
                normals = mesh.vertex_normals(verts, faces).contiguous()
            tmap = mesh.texel_map(uvs, uv_faces, size)
            points, point_normals = mesh.texel_surface(tmap, verts, faces, normals)
            state = mesh.texture_state(tmap, 3)
            torch.cuda.synchronize(dev)
            times["texel_map"] = time.perf_counter() - t0
            for pose in poses:
                t0 = time.perf_counter()
                rgb = self.render_fitting(H, W, K, chunk=chunk, c2w=pose, ndc=False, shapeCodes=shapeCodes, uvCodes=uvCodes, expType=expType,
                                          expCodes=expCodes, **render_kwargs)[0]
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                r = mesh.rasterize(verts, faces, H, W, K, pose)
                frame = mesh.depth_frame(r["depth"], r["mask"], "empty")
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                mesh.bake_integrate(state, points, rgb.reshape(H, W, 3).contiguous(), frame, K, pose, point_normals, depth_tol=depth_tol,
                                    cos_min=cos_min, power=power)
                shares.append(r["mask"].float().mean())
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
                times["render"] += t1 - t0
                times["rasterize"] += t2 - t1
                times["integrate"] += t3 - t2
            t0 = time.perf_counter()
            image = mesh.texture_image(state, tmap, blend, 0.0, int(dilate))
            torch.cuda.synchronize(dev)
            times["resolve"] = time.perf_counter() - t0
        stats = dict(image["counts"])
        stats.update({k: tmap["counts"][k] for k in ("covered", "multi", "degenerate", "faces_without_texels")})
        stats.update(remaining=int(image["remaining"]), hit_share=[float(s) for s in torch.stack(shares).cpu()], times=times, blend=blend,
                     depth_tol=depth_tol, cos_min=cos_min, power=power, size=tmap["size"], dilate=int(dilate))
        self.bake_state, self.bake_stats, self.bake_map = state, stats, tmap
        self.check_launches(block=True)
        return image["texture"], image["valid"], stats

    def render_path_mesh(self, render_poses, hwf, K, verts, faces, colors=None, savedir=None, znear=1e-3, ambient=0.3, near=None, far=None,
                         name=None, texture=None, uvs=None, uv_faces=None):
        """One :meth:`render_mesh` frame per pose: a turntable of an exported mesh at the cost of a z-buffer.  With ``savedir`` two 8-bit
        PNGs per pose go through the ``PngSink``: ``<stem>_mesh.png`` (``rgb``) and ``<stem>_mesh_depth.png`` (``(depth - near) / (far -
        near)`` in grey, black where nothing is hit; ``near`` / ``far`` default to the least and greatest depth of the frame); ``stem`` as
        in :meth:`render_path_geometry`.  A pose whose two files exist is skipped.  Returns a dict of numpy arrays stacked over the
        rendered poses — ``rgb``, ``depth``, ``mask``, ``face`` — with ``rendered`` and ``skipped``, the lists of pose numbers.
        ``texture`` / ``uvs`` / ``uv_faces`` are :meth:`render_mesh`'s: a textured turntable."""
        height, width, _ = hwf
        height, width = int(height), int(width)
        if (near is None) != (far is None) or (near is not None and not _scalar(far) > _scalar(near)):
            raise lib.MofaError(f"render_path_mesh: near = {near}, far = {far} (want both or neither, far > near)")

        def frame(i, paths, sink):
            rgb, depth, mask, ex = self.render_mesh(height, width, K, render_poses[i][:3, :4], verts, faces, colors=colors, znear=znear,
                                                    ambient=ambient, texture=texture, uvs=uvs, uv_faces=uv_faces)
            if paths is not None:
                if near is None:
                    hit = depth[mask]
                    lo, hi = (hit.min(), hit.max()) if hit.numel() else (depth.new_zeros(()), depth.new_ones(()))
                    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
                else:
                    lo, span = depth.new_tensor(_scalar(near)), depth.new_tensor(_scalar(far) - _scalar(near))
                grey = ((depth - lo) / span) * mask.to(torch.float32)
                sink.submit(paths[0], rgb)
                sink.submit(paths[1], grey[..., None].expand(height, width, 3))
            return {"rgb": rgb, "depth": depth, "mask": mask, "face": ex["face"]}

        return self._pose_loop(len(render_poses), name, savedir, ("_mesh.png", "_mesh_depth.png"), frame)

    def build_occupancy(self, networks, *, bounds, resolution, threshold, shapeCodes, expType=20, expCodes=None, dilate=1, netchunk=None):
        """Occupancy grid for ``render_rays(..., occupancy=...)``: the density of each of ``networks`` (one network or a sequence,
        normally coarse and fine) from :meth:`query_density` on the lattice ``bounds`` x ``resolution``; a cell is occupied iff one of
        its 8 corner samples is ``> threshold`` in ANY of the networks (the union), and then iff a cell within Chebyshev distance
        ``dilate`` (0 .. 8 cells) was (``occupancy.occupancy_from_grid``).  ``threshold`` has no default: no density level of a trained
        MoFaNeRF has been measured.  Everything outside ``bounds`` counts as empty, so the bounds must hold the head.

        The grid belongs to the shape and expression codes it was built with — density does not depend on the texture code, the view
        direction or the camera pose (models/model.py:121-128), so one grid serves every frame of that identity and expression.  With
        ``ndc=True`` the renderer's points are NDC points and ``bounds`` must be NDC bounds."""
        from . import mesh, occupancy
        nets = list(networks) if isinstance(networks, (list, tuple)) else [networks]
        if not nets or any(n is None for n in nets):
            raise lib.MofaError("build_occupancy: networks must be one network or a non-empty sequence of networks")
        threshold = occupancy._check_threshold(threshold, "build_occupancy")
        dilate = occupancy._check_dilate(dilate)
        _, lo, step = mesh.grid_spec(bounds, resolution)
        grids = [self.query_density(n, bounds=bounds, resolution=resolution, shapeCodes=shapeCodes, expType=expType, expCodes=expCodes,
                                    netchunk=netchunk) for n in nets]
        with torch.no_grad():
            return occupancy.occupancy_from_grids(grids, threshold, lo, step, dilate)

    def extract_mesh(self, network, *, bounds, resolution, level, shapeCodes, expType=20, expCodes=None, uvCodes=None, colors=False,
                     netchunk=None, brick=None, refine=0, normals=None, components=None, simplify=None, placement="quadric", simplify_error=False,
                     smooth=None, smooth_weights="uniform"):
        """Triangle mesh of the face: ``{density >= level}`` over the grid of :meth:`query_density`, by marching tetrahedra on the GPU
        (``mofa_iso_count`` / ``mofa_iso_emit``).  Returns ``(verts [V,3] float32, faces [F,3] int32)`` — watertight, normals
        ``(v1 - v0) x (v2 - v0)`` toward lower density — plus, with ``colors=True`` (needs ``uvCodes``), ``colors [V,3]`` in [0,1]:
        ``sigmoid(raw[..., :3])`` of the full ``run_network`` at each vertex, looking straight at the surface (view direction = minus the
        area-weighted vertex normal).  ``level`` has no default: no iso-level of a trained MoFaNeRF has been measured.  A density grid
        with a non-finite value raises ``MofaError``.

        ``brick = B`` (4, 8 or 16; ``(n - 1) % B == 0`` on every axis) takes the narrow-band path (``mesh.band_surface``): the density is
        evaluated only at the brick corners and in the bricks the surface passes through, in chunks of ``netchunk`` points, with the
        folded codes of :meth:`query_density`.  Every surface component that passes through a brick whose corners straddle the level
        comes out exactly as on the dense grid, its vertices numbered by brick (``self.mesh_stats["edge_ids"]`` gives each vertex's edge
        id; ordering by it gives the dense numbering); smaller components are missed.  ``self.mesh_stats`` keeps the statistics of the
        last band extraction.

        ``refine = k`` (1 .. 20, on either path) then moves every vertex along its lattice edge onto the level by k bisection steps on the
        network's density (``mesh.refine_vertices``: (2 + k) V more density evaluations, the placement of a grid ``2^k`` times finer along
        each edge; faces and numbering unchanged).  ``normals="density"`` appends ``normals [V,3]`` as the last element of the result: unit
        normals of the density field by central differences at half a grid step (``mesh.density_normals``, 6 V evaluations; (0, 0, 0)
        where the gradient vanishes), and the colours then look along them (along the face normals where they are zero);
        ``normals="faces"`` appends ``mesh.vertex_normals`` instead.  With either, ``self.mesh_stats`` is filled on the dense path too:
        ``edge_ids``, ``refine`` (``mesh.refine_vertices``' statistics) and ``zero_normals``.  With both at their defaults nothing of
        this is launched.

        ``components="largest"`` or ``components=n`` removes floaters right after the extraction, before refinement, normals and colours
        (which then run on the kept vertices only): the mesh's connected components are labelled (``mesh.components``) and only the one
        with the most faces, or every one with at least ``n`` faces, is kept (``mesh.keep_components``; kept vertices and faces stay in
        their order).  ``self.mesh_stats["components"]`` then holds the statistics of the unfiltered mesh plus ``kept`` (the mask), and
        ``self.mesh_stats["edge_ids"]`` is filtered with the vertices.  ``None`` launches nothing and returns the same bytes as before.

        ``simplify=m`` (an integer >= 2) simplifies the mesh by vertex clustering with quadric-error representatives (``mesh.simplify``) on
        cells of ``m`` grid steps per axis from the grid's ``lo``, so the clusters are lattice-aligned; ``placement="mean"`` is the plain
        clustering baseline.  It runs after ``components=`` and ``refine=`` (refinement needs the edge ids, which do not survive: the
        ``edge_ids`` entry of ``self.mesh_stats`` is dropped) and before ``normals=`` and ``colors=``, which are network evaluations at
        vertex positions and so run on the fewer vertices (``self.mesh_stats["normal_evaluations"]`` / ``["color_evaluations"]`` count
        them); ``normals="faces"`` is computed on the simplified mesh.  ``self.mesh_stats["simplify"]`` keeps ``mesh.simplify``'s
        statistics.  The result is closed where the input is, but not necessarily manifold.  ``None`` launches nothing and returns the
        same bytes as before.  What it does to a trained face has not been measured.

        ``simplify_error=True`` (needs ``simplify=``) measures what the simplification cost: the surface distance, both ways
        (``mesh.surface_distance``), between the unsimplified mesh — after ``components=`` and ``refine=`` — and the simplified one, sampled at
        one grid step (the smallest of the three).  The result goes to ``self.mesh_stats["simplify_error"]``; ``mesh_stats["simplify"]``
        keeps its shape.  ``False`` launches nothing and adds no key.

        ``smooth=n`` (an integer >= 1) runs ``n`` iterations of Taubin smoothing over the vertices (``mesh.smooth`` with its defaults:
        lam 0.5, mu -0.53, the boundary fixed; ``smooth_weights`` is ``"uniform"`` or ``"cotangent"``): a low-pass filter for the
        lattice-shaped staircase noise of the extraction.  It runs after ``components=``, ``refine=`` and ``simplify=`` and before
        ``normals=`` and ``colors=``, which are evaluated at vertex positions and so see the smoothed ones.  Smoothing moves vertices OFF
        the level set, and ``refine`` cannot run after it (it needs the vertices on their lattice edges: the ``edge_ids`` entry of
        ``self.mesh_stats`` is dropped, as after ``simplify=``).  Faces and numbering stay.  ``self.mesh_stats["smooth"]`` keeps
        ``mesh.smooth``'s statistics.  ``None`` launches nothing, adds no key and returns the same bytes as before.  What it does to a
        trained face has not been measured."""
        from . import mesh
        if smooth is not None and not (isinstance(smooth, (int, np.integer)) and not isinstance(smooth, (bool, np.bool_)) and smooth >= 1):
            raise lib.MofaError(f"extract_mesh: smooth = {smooth!r} (want None or an integer >= 1: Taubin iterations)")
        if smooth_weights not in ("uniform", "cotangent"):
            raise lib.MofaError(f"extract_mesh: smooth_weights = {smooth_weights!r} (want 'uniform' or 'cotangent')")
        if simplify_error and simplify is None:
            raise lib.MofaError("extract_mesh: simplify_error=True measures a simplification; it needs simplify=")
        if simplify is not None and not (isinstance(simplify, (int, np.integer)) and not isinstance(simplify, (bool, np.bool_)) and simplify >= 2):
            raise lib.MofaError(f"extract_mesh: simplify = {simplify!r} (want None or an integer >= 2: grid steps per cell)")
        if placement not in ("quadric", "mean"):
            raise lib.MofaError(f"extract_mesh: placement = {placement!r} (want 'quadric' or 'mean')")
        if components is not None and components != "largest" and not (isinstance(components, (int, np.integer)) and
                                                                       not isinstance(components, (bool, np.bool_)) and components >= 1):
            raise lib.MofaError(f"extract_mesh: components = {components!r} (want None, 'largest' or a face count >= 1)")
        if level is None or not np.isfinite(float(level)):
            raise lib.MofaError(f"extract_mesh: level must be a finite number (got {level})")
        if colors and uvCodes is None:
            raise lib.MofaError("extract_mesh: colors=True needs uvCodes (the texture code the colours are evaluated with)")
        if normals not in (None, "density", "faces"):
            raise lib.MofaError(f"extract_mesh: normals = {normals!r} (want None, 'density' or 'faces')")
        if refine != int(refine) or not 0 <= int(refine) <= mesh.MAX_REFINE:
            raise lib.MofaError(f"extract_mesh: refine = {refine} (want an integer 0 .. {mesh.MAX_REFINE})")
        refine = int(refine)
        extra = refine > 0 or normals is not None
        res, lo, step = mesh.grid_spec(bounds, resolution)
        if brick is None:
            grid = self.query_density(network, bounds=bounds, resolution=resolution, shapeCodes=shapeCodes, expType=expType,
                                      expCodes=expCodes, netchunk=netchunk)
        with torch.no_grad():
            if brick is None and not extra and components is None and simplify is None and smooth is None:
                verts, faces = mesh.iso_surface(grid, float(level), lo, step)
            elif brick is None:
                verts, faces, edge_ids = mesh.iso_surface(grid, float(level), lo, step, edge_ids=True)
                self.mesh_stats = {"edge_ids": edge_ids}
            else:
                verts, faces = self._band_mesh(network, res, lo, step, float(level), int(brick), shapeCodes, expType, expCodes, netchunk)
            if components is not None:
                stats = mesh.components(verts, faces)
                stats["kept"] = mesh.select_components(stats, components)
                verts, faces, self.mesh_stats["edge_ids"] = mesh.keep_components(verts, faces, stats, stats["kept"], self.mesh_stats["edge_ids"])
                self.mesh_stats["components"] = stats
            nrm = None
            if simplify is not None or smooth is not None:
                if refine:
                    verts, _ = self._refine_mesh(network, verts, faces, res, lo, step, float(level), refine, None, shapeCodes, expType,
                                                 expCodes, netchunk)
                if simplify is not None:
                    cell = (np.float32(int(simplify)) * np.asarray(step, dtype=np.float32)).astype(np.float32)
                    full = (verts.contiguous(), faces.contiguous())
                    verts, faces, self.mesh_stats["simplify"] = mesh.simplify(full[0], full[1], cell, origin=lo, placement=placement)
                    if simplify_error:
                        self.mesh_stats["simplify_error"] = mesh.surface_distance(full[0], full[1], verts, faces,
                                                                                  float(np.min(np.asarray(step, dtype=np.float32))))
                    del full
                if smooth is not None:
                    verts, self.mesh_stats["smooth"] = mesh.smooth(verts.contiguous(), faces.contiguous(), iterations=int(smooth),
                                                                   weights=smooth_weights)
                self.mesh_stats.pop("edge_ids", None)
                if normals is not None:
                    verts, nrm = self._refine_mesh(network, verts, faces, res, lo, step, float(level), 0, normals, shapeCodes, expType,
                                                   expCodes, netchunk)
            elif extra:
                verts, nrm = self._refine_mesh(network, verts, faces, res, lo, step, float(level), refine, normals, shapeCodes, expType,
                                               expCodes, netchunk)
            if normals == "density" and isinstance(self.mesh_stats, dict):
                self.mesh_stats["normal_evaluations"] = 6 * int(verts.shape[0])
            if colors and isinstance(self.mesh_stats, dict):
                self.mesh_stats["color_evaluations"] = int(verts.shape[0])
            tail = () if nrm is None else (nrm,)
            if not colors:
                return (verts, faces) + tail
            rgb = torch.empty(0, 3, dtype=torch.float32, device=verts.device)
            if verts.shape[0]:
                vd = -(nrm if normals == "faces" else mesh.vertex_normals(verts, faces))
                if normals == "density":                 # look along the density normal; the faces' where the gradient vanishes
                    vd = torch.where((nrm != 0).any(-1, keepdim=True), -nrm, vd)
                vd = vd.contiguous()
                self.decoding_texCodes = uvCodes.to(verts.device)
                keep, self.netchunk = self.netchunk, int(netchunk if netchunk is not None else self.netchunk)
                try:
                    raw = self.run_network(verts[:, None, :], vd, network)
                finally:
                    self.netchunk = keep
                rgb = torch.sigmoid(raw[:, 0, :3])
        self.check_launches(block=True)
        return (verts, faces, rgb) + tail

    def _band_mesh(self, network, res, lo, step, level, brick, shapeCodes, expType, expCodes, netchunk):
        """extract_mesh's narrow-band path: mesh.band_surface over HipNet.density_points; the statistics go to self.mesh_stats."""
        from . import mesh
        h, _, chunk, folded = self._density_setup("extract_mesh", network, shapeCodes, expType, expCodes, netchunk)

        def density(pts):
            out = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
            h.density_points(pts, out, folded)
            return out

        verts, faces, edge_ids, stats = mesh.band_surface(density, res, lo, step, level, brick, chunk,
                                                          verify=lambda: self.check_launches(block=True))
        stats["edge_ids"] = edge_ids
        self.mesh_stats = stats
        return verts, faces

    def _refine_mesh(self, network, verts, faces, res, lo, step, level, refine, normals, shapeCodes, expType, expCodes, netchunk):
        """extract_mesh's ``refine`` / ``normals``: mesh.refine_vertices and mesh.density_normals over HipNet.density_points with the
        folded codes of query_density, on the edges in self.mesh_stats["edge_ids"]; the statistics join self.mesh_stats (``refine``,
        ``zero_normals``).  Returns (verts, normals or None)."""
        from . import mesh
        h, _, chunk, folded = self._density_setup("extract_mesh", network, shapeCodes, expType, expCodes, netchunk)

        def density(pts):
            out = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
            h.density_points(pts, out, folded)
            return out

        def verify():
            self.check_launches(block=True)

        if refine:
            verts, self.mesh_stats["refine"] = mesh.refine_vertices(density, self.mesh_stats["edge_ids"], res, lo, step, level, refine, chunk,
                                                                    verify=verify)
        nrm = None
        if normals == "density":
            nrm, self.mesh_stats["zero_normals"] = mesh.density_normals(density, verts, step, chunk=chunk, verify=verify)
        elif normals == "faces":
            nrm = mesh.vertex_normals(verts, faces)
        return verts, nrm


myRenderer = Renderer   # the reference's class name
