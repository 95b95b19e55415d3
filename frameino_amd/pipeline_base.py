"""What the Wan and the CogVideoX FrameINO pipelines share on the host: the diffusers-style conveniences, `encode_prompt`, the
pre-launch checks, the sample-by-sample run of a batch, the image pre/post-processing and the loop driver.

The loop.  A pipeline expresses one denoise step as `_step(st)` on static device buffers `st` (its `make_state`): no host sync, no
data-dependent shape; timestep / dt / coefficient rows live in device slots.  `_run_steps` drives it: it replays ONE captured step
from a hipGraph (frameino_amd/graph_step.py: step 0 eager, step 1 captured, the rest replays) whenever the loop is capturable --
no per-step callback, no step cache, no per-step window decision, the built-in attention processors, a parallel plan whose
collectives this runtime captures -- and per step it sets `current_timestep`, lets the pipeline refresh its device slots
(`_refresh_slots`: device-to-device copies, no host sync), runs the step and hands the result to the pipeline's callback handling
(`_after_step`).  `use_hip_graph = False` keeps the eager loop, `True` makes a loop that cannot be captured an error.  However the
loop ends -- a step or a callback that raises included -- `current_timestep` goes back to None and the captured graph is dropped:
a graph that holds a captured all-to-all must die before the process group does (graph_step.StepGraph.close).

Every check (`_loop_checks`: step cache, window attention, guider -- in that order) runs before any launch.  The loop state is
one sample's, so a batch runs sample by sample (`_sample_by_sample`); with a step cache every sample starts from fresh state.
What the loop has to know about a cache it asks the cache's policy (step_cache._CachePolicy: `loop_begins`,
`reads_timestep_on_host`)."""
from contextlib import nullcontext  # noqa: F401  (the pipelines' null context)

import numpy as np
import torch

from . import graph_step
from .guiders import GuiderPipelineMixin
from .lora import LoraPipelineMixin
from .window_attention import window_attention_runs_eagerly


class VideoProcessor:
    """The two diffusers VideoProcessor calls the pipelines make (Wan :767, :927); host-side pre/post-processing."""

    def __init__(self, vae_scale_factor=16):
        self.vae_scale_factor = vae_scale_factor

    def preprocess(self, image, height, width):
        """a PIL image or a list of them (resized, stacked) or a tensor [C, H, W] / [B, C, H, W] in [0, 1] or [-1, 1]
        -> [B, C, H, W] in [-1, 1]"""
        import PIL.Image
        if isinstance(image, (PIL.Image.Image, list)):
            arrs = [np.asarray(im.resize((width, height), resample=PIL.Image.LANCZOS)).astype(np.float32) / 255.0
                    for im in (image if isinstance(image, list) else [image])]
            arrs = [a[..., None] if a.ndim == 2 else a for a in arrs]
            return 2.0 * torch.from_numpy(np.stack(arrs).transpose(0, 3, 1, 2).copy()) - 1.0
        if isinstance(image, torch.Tensor):
            t = image if image.ndim == 4 else image[None]
            return t if t.min() < 0 else 2.0 * t - 1.0
        raise ValueError(f"`image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is {type(image)}")

    def postprocess_video(self, video, output_type="np"):
        v = (video.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)       # [B, F, C, H, W]
        if output_type == "pt":
            return v
        if output_type == "np":
            return v.permute(0, 1, 3, 4, 2).cpu().numpy()
        if output_type == "pil":
            import PIL.Image
            arr = (v.permute(0, 1, 3, 4, 2).cpu().numpy() * 255).round().astype("uint8")
            return [[PIL.Image.fromarray(f) for f in vid] for vid in arr]
        raise ValueError(f"unsupported output_type {output_type}")


def tr_default_procs(transformer):
    """the built-in processors run only this library's kernels: capturable.  A user-installed processor may do anything
    (host syncs included), so its loop stays eager unless `use_hip_graph = True` asks for the capture"""
    f = getattr(transformer, "_default_processors", None)
    return bool(f()) if callable(f) else True


class DenoisePipelineBase(LoraPipelineMixin, GuiderPipelineMixin):
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]
    _negative_batch_message = None       # the words of `encode_prompt`'s batch-size ValueError, as the mirrored reference has them
    _interrupt = False
    _current_timestep = None
    use_hip_graph = None                 # None: graph replay whenever the loop is capturable; False: eager; True: capture or raise

    # ---- diffusers-style conveniences ----
    @property
    def _execution_device(self):
        return self.transformer.device

    @property
    def interrupt(self):
        return self._interrupt

    @property
    def current_timestep(self):
        return self._current_timestep

    def enable_model_cpu_offload(self, *a, **k):      # reference app.py:163 -- unnecessary with 288 GB of HBM
        return self

    def to(self, device):
        for m in (self.transformer, self.vae, self.text_encoder):
            if m is not None and hasattr(m, "to"):
                m.to(device)
        return self

    def maybe_free_model_hooks(self):
        # diffusers resets every component's stateful cache here, at the end of each call
        reset = getattr(self.transformer, "_reset_stateful_cache", None)
        if callable(reset):
            reset()

    # ---- text ----
    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance=True, num_videos_per_prompt=1,
                      prompt_embeds=None, negative_prompt_embeds=None, max_sequence_length=226, device=None, dtype=None):
        """reference Wan :258-337, CogVideoX :269-348"""
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        bsz = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        if prompt_embeds is None:
            prompt_embeds = self._get_t5_prompt_embeds(prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt = bsz * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got "
                                f"{type(negative_prompt)} != {type(prompt)}.")
            if bsz != len(negative_prompt):
                raise ValueError(self._negative_batch_message.format(negative_prompt=negative_prompt, prompt=prompt,
                                                                     n=len(negative_prompt), bsz=bsz))
            negative_prompt_embeds = self._get_t5_prompt_embeds(negative_prompt, num_videos_per_prompt,
                                                                max_sequence_length, device, dtype)
        return prompt_embeds, negative_prompt_embeds

    # ---- the checks before any launch ----
    def _step_cache_check(self, batch=1):
        """the limits of the step caches (first-block caching, Pyramid Attention Broadcast, TaylorSeer, FasterCache, MagCache,
        TeaCache, region-adaptive sampling), checked before any work (and before any collective: a parallel plan and the cache are
        configured by the same script on every rank, so every rank raises).  -> whether one is enabled: the loop then runs eagerly"""
        if not getattr(self.transformer, "is_cache_enabled", False):
            return False
        policy = self.transformer._step_cache_policy        # (label, batch rule and capture reason: stated once, by the cache)
        if getattr(self, "parallel", None) is not None:
            raise NotImplementedError(f"{policy.label} runs on one GPU; this pipeline has a parallel plan")
        if batch > 1 and not policy.batched:
            # (the others decide from the step counter and the timestep alone: the samples of a batch, run one at a time from
            # fresh state, decide as diffusers' joint run does)
            raise NotImplementedError(f"{policy.label} with a batch (a list of prompts, num_videos_per_prompt > 1): diffusers "
                                      f"decides jointly over the batch, this pipeline runs the samples one at a time")
        if self.use_hip_graph is True:
            raise policy.capture_refusal()
        return True

    def _window_attention_check(self):
        """the limits of window / sparse attention (`enable_window_attention` of the transformer), checked before any work.  ->
        whether the loop must run eagerly: with a timestep range the host decides per step whether the windows apply."""
        if getattr(self.transformer, "is_window_attention_enabled", False) and getattr(self, "parallel", None) is not None:
            raise NotImplementedError("window attention runs on one GPU; this pipeline has a parallel plan")
        if getattr(self.transformer, "is_sparse_attention_enabled", False) and getattr(self, "parallel", None) is not None:
            raise NotImplementedError("sparse attention runs on one GPU; this pipeline has a parallel plan")
        return window_attention_runs_eagerly(self.transformer, self.use_hip_graph)

    def _loop_checks(self, batch):
        """-> (a step cache is on, window attention needs the eager loop, the guider's config or None); with a cache, its state is
        fresh afterwards"""
        checks = self._step_cache_check(batch), self._window_attention_check(), self._guider_check()
        if checks[0]:
            self.transformer._reset_stateful_cache()
        return checks

    # ---- the loop ----
    @staticmethod
    def _sample_by_sample(denoise_one, latents, tensors, generator=None):
        """A batch, run as `denoise_one(i, latents_i, tensors_i, generator_i)` per sample: the samples of a batched loop never meet
        (per-sample attention, per-sample guidance), so every row equals the single call on that row's noise, prompt and
        conditions.  Tensors given with batch 1 (or None) are shared; a list of generators is indexed."""
        def row(t, i):
            return t if t is None or t.shape[0] == 1 else t[i:i + 1]
        outs = []
        for i in range(latents.shape[0]):
            gi = generator[i] if isinstance(generator, (list, tuple)) else generator
            outs.append(denoise_one(i, latents[i:i + 1], [row(t, i) for t in tensors], gi))
        return torch.cat(outs, dim=0)

    def _refresh_slots(self, st, i):
        """before step i: this step's rows of the schedule into the device slots of `st` (device-to-device: no host sync)"""
        raise NotImplementedError

    def _after_step(self, st, i, t, callback, tensor_inputs):
        """after step i of a loop with a `callback_on_step_end`: call it, and take back what it replaced"""
        raise NotImplementedError

    def _run_steps(self, st, timesteps, cached, win_eager, plan=None, callback=None, tensor_inputs=None):
        """The loop over `timesteps` on the state `st` (module docstring)."""
        tr, explicit = self.transformer, self.use_hip_graph is True
        policy = tr._step_cache_policy if cached else None
        host_ts = None
        if policy is not None:
            policy.loop_begins(tr._step_cache_config, len(timesteps))
            if policy.reads_timestep_on_host:      # a host copy of the schedule, taken once, keeps those reads off the device
                host_ts = timesteps.cpu()
        capturable = (callback is None and st.lat.is_cuda and not cached and not win_eager
                      and (explicit or tr_default_procs(tr)) and graph_step.groups_capturable(plan, explicit))
        stepper = graph_step.StepGraph(lambda: self._step(st), self.use_hip_graph, capturable, len(timesteps),
                                       graph_step.capture_error_mode(plan))
        try:
            for i, t in enumerate(timesteps):
                if self._interrupt:
                    continue
                self._current_timestep = t if host_ts is None else host_ts[i]
                self._refresh_slots(st, i)
                self._guider_begin_step(st.guider, i)
                stepper.step()
                if callback is not None:
                    self._after_step(st, i, t, callback, tensor_inputs)
        finally:
            self._current_timestep = None
            stepper.close()
