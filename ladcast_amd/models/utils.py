"""Host-side helpers of the denoising objective.

``Karras_sigmas_lognormal`` keeps the reference's public surface (models/utils.py: constructor keywords, call signature, returned
indices), restated here: a log-normal draw of one noise level per sample, snapped to the nearest entry of the scheduler's training
schedule.  All arithmetic is fp32 torch on the CPU tensor of training sigmas, so a seeded generator yields the same indices as the
reference's sampler (pinned by tests/golden/denoise_loss_ref.npz).
"""
from __future__ import annotations

import torch


class Karras_sigmas_lognormal:
    """Draws indices into a scheduler's training sigmas.

    ln(sigma) ~ N(mean_k, std_k^2), where (mean_k, std_k) walk linearly from (P_mean_start, P_std_start) at step 0 to
    (P_mean_end, P_std_end) at step num_max_steps - 1 and stay there.  `sigmas` is `scheduler.sigmas`: the descending training
    schedule followed by the scheduler's appended 0, which is never a candidate."""

    def __init__(self, sigmas, P_mean_start=-1.2, P_std_start=1.2, P_mean_end=1.2, P_std_end=1.7, num_max_steps=50000):
        self.sigmas = sigmas
        self.num_max_steps = int(num_max_steps)
        self.P_mean_start, self.P_mean_end = P_mean_start, P_mean_end
        self.P_std_start, self.P_std_end = P_std_start, P_std_end
        # (2, num_max_steps) fp32: row 0 the means, row 1 the standard deviations of ln(sigma) per training step
        self._lognormal = torch.stack([torch.linspace(P_mean_start, P_mean_end, self.num_max_steps),
                                       torch.linspace(P_std_start, P_std_end, self.num_max_steps)])

    def lognormal_parameters(self, cur_step):
        """(mean, std) of ln(sigma) at training step `cur_step`, as fp32 0-dim tensors"""
        k = min(int(cur_step), self.num_max_steps - 1)
        return self._lognormal[0, k], self._lognormal[1, k]

    def __call__(self, batch_size, cur_step, generator=None, device="cpu"):
        mean, std = (v.to(device) for v in self.lognormal_parameters(cur_step))
        z = torch.randn([batch_size, 1, 1, 1], device=device, generator=generator)  # the shape fixes how the generator is consumed
        drawn = torch.exp(z * std + mean).reshape(batch_size, 1)
        candidates = self.sigmas[:-1].to(device).reshape(1, -1)
        return (candidates - drawn).abs().argmin(dim=1)  # first index on a tie
