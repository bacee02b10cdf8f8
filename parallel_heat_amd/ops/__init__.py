"""Tensor-level stencil kernels (gfx950 HIP on ROCm tensors, OpenMP oracle on CPU tensors)."""
from .stencil import (MAX_BOX_COPIES, Field, Gate, Geom, TbTuning, TbVariant, checksum, coarse,
                      coarse_dims, coarse_plan, set_coarse_max_waves, copy_boxes, fill_edge_ghosts, fill_insulated_ghosts, init_field, judge,
                      lds_step, mfma_step, naive_step, pack, residual, resid_value,
                      set_tb_tuning, tb_stamps, tb_step, tb_tuning, unpack)
from .stencil import refine, refine_axis, refine_plan, set_refine_max_waves
from .stencil import (set_source_max_waves, set_source_nontemporal, source_plan,  # noqa: F401
                      source_step)
from .stencil import (set_source_tb_max_waves, source_tb_launches, source_tb_plan,  # noqa: F401
                      source_tb_step)

__all__ = ["Field", "Geom", "TbTuning", "TbVariant", "init_field", "lds_step", "mfma_step",
           "naive_step", "tb_step", "tb_stamps", "tb_tuning", "set_tb_tuning", "pack", "unpack",
           "residual", "resid_value", "fill_insulated_ghosts", "fill_edge_ghosts",
           "copy_boxes", "MAX_BOX_COPIES", "judge", "Gate", "checksum", "coarse", "coarse_dims",
           "coarse_plan", "set_coarse_max_waves", "refine", "refine_axis", "refine_plan",
           "set_refine_max_waves", "source_step", "source_plan", "set_source_max_waves",
           "set_source_nontemporal", "source_tb_step", "source_tb_plan",
           "set_source_tb_max_waves", "source_tb_launches"]
