"""The hand-over into the discrete language stage: the status centres of every Gaussian, on the MI355X
(csrc/deform_lang.hip k_centers_from_field, csrc/centers.hip; C-ABI include/lsr_centers.h).

Replaces GaussianModel.generate_multi_feature_centers (scene/gaussian_model.py:804-845) and the
discrete branch of training_setup (:226-231):
  init_from_stage 'fine-base'   every centre = the unit-normalised static feature + N(0, 0.05) noise
  init_from_stage 'fine-lang'   the language field at `samples` random times per Gaussian, then one
                                k-means per Gaussian.  The reference stacks [P, 100, D] on the host and
                                fits sklearn's KMeans P times; here one fused kernel samples the times,
                                runs lang_deform and clusters the rows without writing them out.
Two quirks of the reference are not reproduced silently:
  * :830 takes [-1] of the field's outputs, which is coff (None under init_centers=True), so its
    'fine-lang' branch cannot run as released.  The language output (index -2) is what is clustered.
  * :230 applies permute(0, 2, 1) before flattening while the field views the tensor as
    (P, centers, D) (scene/deformation.py:158): with centers == D == 3 the shapes pass and the centres
    arrive transposed.  The layout here is (P, centers, D), the one the discrete field reads;
    reference_permute=True gives the reference's.
The k-means is deterministic (maximin seeding, Lloyd, fixed summation order: include/lsr_centers.h);
sklearn's k-means++ random stream is not reproduced.  There is no CPU fallback for the sampled path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from deformation import COFF, HEADS, LANG_DISCRETE, LANG_NORESNET, LANG_RESIDUAL, DeformationField
from diff_gaussian_rasterization import _lib


def _device_f32(t, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name}: a float32 CUDA tensor is required")
    return t.detach().contiguous()


def _outputs(P: int, k: int, D: int, device):
    k_, D_ = max(k, 0), max(D, 0)
    return (torch.empty(P, k_, D_, device=device), torch.empty(P, k_, dtype=torch.int32, device=device),
            torch.empty(P, device=device), torch.empty(P, dtype=torch.int32, device=device))


def _out_ptrs(B, outs):
    centers, counts, inertia, iters = outs
    return (B.ptr(centers, "centers"), B.ptr(counts, "counts", torch.int32), B.ptr(inertia, "inertia"),
            B.ptr(iters, "iters", torch.int32))


@torch.no_grad()
def kmeans_rows(x: torch.Tensor, k: int, max_iter: int = 100):
    """k-means of every row of x [P, S, D] (float32, CUDA) with the algorithm of include/lsr_centers.h.
    Returns (centers [P, k, D], counts [P, k] int32, inertia [P], iters [P] int32)."""
    x = _device_f32(x, "x")
    if x.dim() != 3:
        raise ValueError("x: [P, S, D]")
    P, S, D = x.shape
    centers, counts, inertia, iters = outs = _outputs(P, k, D, x.device)
    B = _lib.Boundary(x.device)
    _lib.check(_lib.load().lsr_centers_kmeans(B.ptr(x, "x"), P, S, D, int(k), int(max_iter), *_out_ptrs(B, outs),
                                              B.stream()), "lsr_centers_kmeans")
    return centers, counts, inertia, iters


def _refuse_narrow(field, what):
    """The centres and the discrete stage exist for the 16-channel / 128-wide field only."""
    if (getattr(field, "channels", 16), getattr(field, "width", 128)) != (16, 128):
        raise ValueError(f"{what}: not supported for a field of output_coordinate_dim {field.channels} / "
                         f"net_width {field.width} (it passes the language through; 16 / 128 only)")


@torch.no_grad()
def sample_centers(field: DeformationField, lang: torch.Tensor, k: int = 3, samples: int = 100, seed: int = 0,
                   times: Optional[torch.Tensor] = None, max_iter: int = 100, debug: bool = False):
    """The centres of every Gaussian's language feature over time: `field` (LANG_RESIDUAL or
    LANG_NORESNET) evaluated on lang / (|lang| + 1e-9) at `samples` times per Gaussian -- `times`
    [P, samples], or the stateless generator of (seed, Gaussian, sample) -- and clustered per Gaussian.
    Returns (centers [P, k, D], counts, inertia, iters); with debug=True also the samples [P, S, D]
    and the times [P, S]."""
    _refuse_narrow(field, "sample_centers")
    lang = _device_f32(lang, "lang")
    if lang.dim() != 2 or lang.shape[1] != field.lang_dim:
        raise ValueError(f"lang: [P, {field.lang_dim}]")
    P, D, S = lang.shape[0], field.lang_dim, int(samples)
    if times is not None:
        times = _device_f32(times, "times")
        if tuple(times.shape) != (P, S):
            raise ValueError(f"times: [{P}, {S}]")
    centers, counts, inertia, iters = outs = _outputs(P, k, D, lang.device)
    B = _lib.Boundary(lang.device)
    xs = torch.empty(P, max(S, 0), D, device=lang.device) if debug else None
    ts = torch.empty(P, max(S, 0), device=lang.device) if debug else None
    _lib.check(_lib.load().lsr_centers_from_field(
        ctypes.byref(field.net), B.ptr(field.workspace, "field.workspace", torch.uint8), P, B.ptr(lang, "lang"),
        B.opt(times, "times"), int(seed) & 0xFFFFFFFF, S, int(k), int(max_iter), *_out_ptrs(B, outs),
        B.opt(xs, "samples"), B.opt(ts, "sample times"), B.stream()), "lsr_centers_from_field")
    return (centers, counts, inertia, iters) + ((xs, ts) if debug else ())


@torch.no_grad()
def init_centers(lang: torch.Tensor, k: int, init_from_stage: str, field: Optional[DeformationField] = None,
                 noise_std: float = 0.05, generator: Optional[torch.Generator] = None, reference_permute: bool = False,
                 **sampling) -> torch.Tensor:
    """The language tensor [P, k * D] a discrete field reads, from the static features lang [P, D].
    'fine-base': torch.normal(mean=lang / (|lang| + 1e-9), std=noise_std) per centre (plain torch, any
    device; `generator` optional).  'fine-lang': sample_centers(field, lang, k, **sampling).
    The layout is (P, k, D) flattened; reference_permute=True applies the reference's
    permute(0, 2, 1) first (scene/gaussian_model.py:230: its quirk, the centres arrive transposed)."""
    if init_from_stage == "fine-base":
        if sampling:
            raise ValueError(f"'fine-base' draws noise, it takes no sampling options: {sorted(sampling)}")
        unit = lang.detach() / (lang.detach().norm(dim=-1, keepdim=True) + 1e-9)
        centers = torch.stack([torch.normal(mean=unit, std=noise_std, generator=generator) for _ in range(k)], dim=1)
    elif init_from_stage == "fine-lang":
        if field is None:
            raise ValueError("'fine-lang' samples the language field: field is required")
        centers = sample_centers(field, lang, k=k, **sampling)[0]
    else:
        raise ValueError(f"init_from_stage {init_from_stage!r}: 'fine-base' or 'fine-lang'")
    if reference_permute:
        centers = centers.permute(0, 2, 1)
    return centers.reshape(centers.shape[0], -1).contiguous()


def discrete_field_from(field: DeformationField, centers: int = 3, seed: int = 0) -> DeformationField:
    """The LANG_DISCRETE field of the same structure: the shared parameters copied, lang_deform.*
    dropped, discrete_coff_generator.* freshly initialised as DeformationField.init_params does."""
    shared = {n: v.clone() for n, v in field.p.items() if not n.startswith(("lang_deform.", COFF + "."))}
    aabb = field.p["grid.aabb"].cpu()
    fresh = DeformationField.init_params(field.resolution, field.multires, aabb, seed=seed, depth=field.depth,
                                         heads=[h for h, on in zip(HEADS, field.head_on) if on],
                                         lang_mode=LANG_DISCRETE, lang_dim=field.lang_dim, centers=centers,
                                         time_pe=field.time_pe)
    shared.update({n: v.to(field.device) for n, v in fresh.items() if n.startswith(COFF + ".")})
    no = [not on for on in field.head_on]
    return DeformationField(shared, field.resolution, field.multires, device=field.device, depth=field.depth,
                            no_dx=no[0], no_ds=no[1], no_dr=no[2], no_do=no[3], no_dshs=no[4],
                            apply_rotation=field.apply_rotation, lang_mode=LANG_DISCRETE, lang_dim=field.lang_dim,
                            centers=centers, time_pe=field.time_pe)


def enter_discrete_stage(step, init_from_stage: str = "fine-base", centers: int = 3, field_seed: int = 0, **kw):
    """The 'fine-lang-discrete' TrainStep that continues a 'fine-lang' one (training_setup's discrete
    branch, scene/gaussian_model.py:226-231): the language group becomes the [P, centers * lang_dim]
    centres (init_centers; **kw are its options) with a fresh Adam, the other groups are handed over
    (the same tensors, moments and step counts: the old step is finished), the field becomes
    discrete_field_from(step.field, centers, field_seed) with a fresh optimizer, and the step's
    switches carry over.  Refuses a language group whose width is not lang_dim, as :227."""
    from gaussian_train import GaussianTrainer
    from train_step import TrainStep
    old, field = step.trainer, step.field
    if field is None:
        raise ValueError("the discrete stage needs the step's deformation field")
    _refuse_narrow(field, "enter_discrete_stage")
    if "language_feature" not in old.params:
        raise ValueError("the step has no language_feature group")
    lang = old.params["language_feature"].detach()
    if lang.shape[1] != field.lang_dim:
        raise ValueError(f"the language group has width {lang.shape[1]}, not lang_dim {field.lang_dim}: the centres "
                         "are made from static features (scene/gaussian_model.py:227)")
    if init_from_stage == "fine-lang":
        if field.lang_mode not in (LANG_RESIDUAL, LANG_NORESNET):
            raise ValueError("init_from_stage 'fine-lang' needs a field that deforms the language")
        kw = dict(kw, field=field)
    feats = init_centers(lang, centers, init_from_stage, **kw)
    params = {n: p.detach() for n, p in old.params.items()}
    params["language_feature"] = feats
    tr = GaussianTrainer(params, old.lrs, percent_dense=old.percent_dense, betas=old.betas, eps=old.eps,
                         deformation_table=old._deformation_table)
    for n in tr.params:
        if n != "language_feature":
            tr.exp_avg[n], tr.exp_avg_sq[n], tr.steps[n] = old.exp_avg[n], old.exp_avg_sq[n], old.steps[n]
    for n in ("xyz_gradient_accum", "denom", "max_radii2D", "_deformation_accum"):
        setattr(tr, n, getattr(old, n))
    tr.xyz_scheduler_args = old.xyz_scheduler_args
    new = TrainStep(tr, discrete_field_from(field, centers, seed=int(field_seed)), bg=step.bg, stage="fine-lang-discrete",
                    sh_degree=step.sh_degree, densify=step.densify, batch_views=step.batch_views,
                    joint_train=step.joint_train, lam=step.lam, beta=step.beta, addcosloss=step.addcosloss,
                    lambda_dssim=step.lambda_dssim, plane_reg=getattr(step, "plane_reg", None))
    deform_lr = next((lr for n, lr in step.field_opt.lr.items() if not n.startswith("grid.")), None)
    for n in new.field_opt.lr:   # the learning rates the old step ran with (the coff head takes the MLPs')
        if n in step.field_opt.lr:
            new.field_opt.lr[n] = step.field_opt.lr[n]
        elif deform_lr is not None:
            new.field_opt.lr[n] = deform_lr
    new.spatial_lr_scale = step.spatial_lr_scale
    for n in ("_deform_sched", "_grid_sched"):
        if hasattr(step, n):
            setattr(new, n, getattr(step, n))
    return new
