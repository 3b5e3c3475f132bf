"""Occupancy grids for culled rendering: the lattice of a density query (``mesh.grid_spec``), thresholded and dilated into one byte per
cell on the GPU (``mofa_occ_cells`` / ``mofa_occ_dilate``), and the per-pass pieces the renderer drives — classification of a pass's
samples, their compaction into explicit points, the scatter of the network's values back (``mofa_occ_classify`` / ``_gather`` /
``_scatter``).

``Renderer.build_occupancy`` builds a grid from the networks' own density; :func:`occupancy_from_grid` takes any density grid
(analytic ones included).  ``render_rays(..., occupancy=grid)`` then runs the networks only on samples whose cell is occupied.
CPU tensors raise ``MofaError``: there is no CPU path.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import lib
from .mesh import _f3

MAX_DILATE = 8      # cells; the kernels' cap (mofa_occ_dilate)


class OccupancyGrid:
    """A device-resident occupancy grid over the lattice ``resolution = (nx,ny,nz)``, sample (i,j,k) at ``lo + (i,j,k) * step``: one
    byte per cell, ``(nx-1, ny-1, nz-1)`` cells.  ``threshold`` / ``dilate`` are what it was built with; ``fraction`` is the occupied
    share of the cells (read from the device once, when the grid is built)."""

    def __init__(self, cells: torch.Tensor, resolution, lo, step, threshold: float, dilate: int, fraction: float):
        self._cells = cells
        self.resolution = tuple(int(n) for n in resolution)
        self.lo = np.asarray(lo, dtype=np.float32).reshape(3).copy()
        self.step = np.asarray(step, dtype=np.float32).reshape(3).copy()
        self.threshold, self.dilate, self.fraction = float(threshold), int(dilate), float(fraction)
        self._lo3, self._step3 = _f3(self.lo), _f3(self.step)

    @property
    def device(self) -> torch.device:
        return self._cells.device

    def cells(self) -> torch.Tensor:
        """The cells as a ``[nx-1, ny-1, nz-1]`` bool tensor on the grid's device (a copy)."""
        return self._cells.bool()

    def __repr__(self):
        return (f"OccupancyGrid(resolution={self.resolution}, lo={self.lo.tolist()}, step={self.step.tolist()}, threshold={self.threshold}, "
                f"dilate={self.dilate}, fraction={self.fraction:.4f}, device={self.device})")


def _check_dilate(dilate) -> int:
    d = int(dilate)
    if d != dilate or d < 0 or d > MAX_DILATE:
        raise lib.MofaError(f"dilate = {dilate}: want an integer number of cells in 0 .. {MAX_DILATE}")
    return d


def _check_threshold(threshold, what: str) -> float:
    if threshold is None or not np.isfinite(float(threshold)):
        raise lib.MofaError(f"{what}: threshold must be a finite number (got {threshold})")
    return float(threshold)


def occupancy_from_grids(grids: Sequence[torch.Tensor], threshold, lo, step, dilate: int = 1) -> OccupancyGrid:
    """The union of the grids' occupied cells, then dilation: see :func:`occupancy_from_grid`.  Every grid has the same shape."""
    threshold = _check_threshold(threshold, "occupancy_from_grid")
    dilate = _check_dilate(dilate)
    if not len(grids):
        raise lib.MofaError("occupancy_from_grid: no grid")
    shape = tuple(grids[0].shape)
    L = lib.load()
    raw = finite = None
    for g in grids:
        if not torch.is_tensor(g) or g.dim() != 3 or tuple(g.shape) != shape:
            raise lib.MofaError(f"occupancy_from_grid: want [nx,ny,nz] grids of one shape, got {getattr(g, 'shape', type(g))} next to {shape}")
        g = g.detach()
        lib.ptr(g)                                            # (device / dtype / layout check)
        st = lib.stream()
        nx, ny, nz = (int(v) for v in shape)
        if min(shape) < 2:
            raise lib.MofaError(f"occupancy_from_grid: grid {nx} x {ny} x {nz} needs at least 2 samples per axis")
        if raw is None:
            raw = torch.empty(nx - 1, ny - 1, nz - 1, dtype=torch.uint8, device=g.device)
        elif g.device != raw.device:
            raise lib.MofaError(f"occupancy_from_grid: grids on {raw.device} and {g.device}")
        lib.check(L.mofa_occ_cells(lib.ptr(g), nx, ny, nz, threshold, int(finite is not None), raw.data_ptr(), st), "mofa_occ_cells")
        ok = torch.isfinite(g).all()
        finite = ok if finite is None else finite & ok
    lo3, st3 = _f3(lo), _f3(step)
    if not all(np.isfinite(v) for v in (*lo3, *st3)) or min(st3) <= 0:
        raise lib.MofaError(f"occupancy_from_grid: lo = {list(lo3)}, step = {list(st3)} (want finite, step > 0)")
    cells, scratch = torch.empty_like(raw), torch.empty_like(raw)
    lib.check(L.mofa_occ_dilate(raw.data_ptr(), nx, ny, nz, dilate, scratch.data_ptr(), cells.data_ptr(), st), "mofa_occ_dilate")
    ok, count = (int(v) for v in torch.stack([finite.long(), cells.sum(dtype=torch.int64)]).cpu())    # the build's one host read
    if not ok:
        raise lib.MofaError("occupancy_from_grid: the density grid holds non-finite values")
    return OccupancyGrid(cells, shape, lo, step, threshold, dilate, count / cells.numel())


def occupancy_from_grid(grid: torch.Tensor, threshold, lo, step, dilate: int = 1) -> OccupancyGrid:
    """Occupancy grid of a density grid ``[nx,ny,nz]`` (float32, GPU) whose sample (i,j,k) sits at ``lo + (i,j,k) * step`` — the
    counterpart of ``mesh.iso_surface``.  Cell (i,j,k) is occupied iff one of its 8 corner samples is ``> threshold``; then a cell is
    occupied iff some cell within Chebyshev distance ``dilate`` (clipped at the borders; 0 .. 8 cells) was.  A non-finite grid value or
    threshold raises ``MofaError``."""
    return occupancy_from_grids([grid], threshold, lo, step, dilate)


class CulledPass:
    """One pass (coarse or fine) of ``R`` rays x ``S`` samples classified against a grid: ``flags [R,S]`` (uint8), ``n_kept`` (the pass's
    one host read), and — after :meth:`gather` — the kept samples' points, view directions and flat sample indices ``r S + s`` in
    ascending order.  :meth:`scatter` writes every element of ``raw [R,S,4]``,
    :meth:`scatter_sigma` every element of a one-float ``sigma [R,S]``."""

    def __init__(self, grid: OccupancyGrid, rays_o, rays_d, z, z_stride: int, S: int):
        L = lib.load()
        self.R, self.S, self.dev = int(rays_o.shape[0]), int(S), rays_o.device
        self.rays_o, self.rays_d, self.z, self.z_stride = rays_o, rays_d, z, int(z_stride)
        n = self.R * self.S
        nbytes = L.mofa_occ_workspace_bytes(n)
        if nbytes == 0:
            raise lib.MofaError(f"occupancy: a pass of {self.R} rays x {self.S} samples is refused (want 1 .. 2^31 - 1 samples; lower chunk)")
        self.flags = torch.empty(self.R, self.S, dtype=torch.uint8, device=self.dev)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        counts = torch.empty(1, dtype=torch.int64, device=self.dev)
        nx, ny, nz = grid.resolution
        lib.check(L.mofa_occ_classify(lib.ptr(rays_o), lib.ptr(rays_d), lib.ptr(z), self.z_stride, self.R, self.S, grid._cells.data_ptr(),
                                      nx, ny, nz, grid._lo3, grid._step3, self.flags.data_ptr(), self._ws.data_ptr(), counts.data_ptr(),
                                      lib.stream()), "mofa_occ_classify")
        self.n_kept = int(counts.cpu())
        self.n_samples = n

    def gather(self, viewdirs) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(pts [n_kept,3], dirs [n_kept,3], index [n_kept] int32)`` of the kept samples."""
        n = self.n_kept
        pts = torch.empty(n, 3, dtype=torch.float32, device=self.dev)
        dirs = torch.empty(n, 3, dtype=torch.float32, device=self.dev)
        index = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n:
            lib.check(lib.load().mofa_occ_gather(lib.ptr(self.rays_o), lib.ptr(self.rays_d), lib.ptr(viewdirs), lib.ptr(self.z), self.z_stride,
                                                 self.R, self.S, self.flags.data_ptr(), self._ws.data_ptr(), n, lib.ptr(pts), lib.ptr(dirs),
                                                 index.data_ptr(), lib.stream()), "mofa_occ_gather")
        return pts, dirs, index

    def scatter(self, raw_kept, raw: torch.Tensor) -> torch.Tensor:
        """``raw [R,S,4]``: the rows of ``raw_kept [n_kept,4]`` at the kept samples, zeros elsewhere."""
        lib.check(lib.load().mofa_occ_scatter(lib.ptr(raw_kept) if self.n_kept else None, self.flags.data_ptr(), self._ws.data_ptr(),
                                              self.n_samples, self.n_kept, lib.ptr(raw), lib.stream()), "mofa_occ_scatter")
        return raw


    def scatter_sigma(self, sigma_kept, sigma: torch.Tensor) -> torch.Tensor:
        """``sigma [R,S]``: the entries of ``sigma_kept [n_kept]`` at the kept samples, zeros elsewhere (the geometry-only render)."""
        lib.check(lib.load().mofa_occ_scatter_sigma(lib.ptr(sigma_kept) if self.n_kept else None, self.flags.data_ptr(), self._ws.data_ptr(),
                                                    self.n_samples, self.n_kept, lib.ptr(sigma), lib.stream()), "mofa_occ_scatter_sigma")
        return sigma


__all__: Sequence[str] = ("OccupancyGrid", "occupancy_from_grid", "occupancy_from_grids", "CulledPass", "MAX_DILATE")
