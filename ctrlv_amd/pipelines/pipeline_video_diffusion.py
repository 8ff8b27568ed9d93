"""VideoDiffusionPipeline (SVD / bbox-predictor sampling, UNet only) on MI355X.

Counterpart of /root/reference/src/ctrlv/pipelines/pipeline_video_diffusion.py:18-315: same `__call__` signature
(:56-80), bbox-latent injection into `image_latents` (:200-206), decoded-frame clamp (:297).
"""
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from .pipeline_utils import PIL, SVDPipelineBase, VaeImageProcessor


class VideoDiffusionPipeline(SVDPipelineBase):
    model_cpu_offload_seq = "image_encoder->unet->vae"
    _callback_tensor_inputs = ["latents"]

    def __init__(self, vae, image_encoder, unet, scheduler, feature_extractor):
        self.register_modules(vae=vae, image_encoder=image_encoder, unet=unet, scheduler=scheduler,
                              feature_extractor=feature_extractor)
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)

    def check_inputs(self, image, height, width):
        pil_ok = PIL is not None and isinstance(image, PIL.Image.Image)
        if not isinstance(image, torch.Tensor) and not pil_ok and not isinstance(image, list):
            raise ValueError(
                "`image` has to be of type `torch.FloatTensor` or `PIL.Image.Image` or `List[PIL.Image.Image]` but is"
                f" {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")

    @torch.no_grad()
    def __call__(
        self,
        image,
        bbox_images: Optional[torch.FloatTensor] = None,
        bbox_conditions: Optional[Dict] = None,
        original_size: Optional[Tuple[int]] = (1242, 375),
        height: int = 576,
        width: int = 1024,
        num_frames: Optional[int] = None,
        num_inference_steps: int = 25,
        min_guidance_scale: float = 1.0,
        max_guidance_scale: float = 3.0,
        fps: int = 7,
        motion_bucket_id: int = 127,
        noise_aug_strength: float = 0.02,
        decode_chunk_size: Optional[int] = None,
        num_videos_per_prompt: Optional[int] = 1,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        latents: Optional[torch.FloatTensor] = None,
        output_type: Optional[str] = "pil",
        callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
        callback_on_step_end_tensor_inputs: List[str] = ["latents"],
        return_dict: bool = True,
        num_cond_bbox_frames: int = 3,
    ):
        # opt-in (CTRLV_PIPELINE=plan): the whole clip as one C call where the plans serve it (pipeline_utils.pipeline_route);
        # with tensor bbox_images that call is ctrlv_pipeline_predict_boxes
        done = self._generate_plan(
            image, None, lambda h, w: self.check_inputs(image, h, w), height=height, width=width, num_frames=num_frames,
            decode_chunk_size=decode_chunk_size, fps=fps, motion_bucket_id=motion_bucket_id,
            noise_aug_strength=noise_aug_strength, num_videos_per_prompt=num_videos_per_prompt, generator=generator,
            latents=latents, latent_channels=self.unet.config.in_channels, min_guidance_scale=min_guidance_scale,
            max_guidance_scale=max_guidance_scale, num_inference_steps=num_inference_steps, control_condition_scale=1.0,
            output_type=output_type, return_dict=return_dict, callback_on_step_end=callback_on_step_end,
            bbox_images=bbox_images, num_cond_bbox_frames=num_cond_bbox_frames)
        if done is not None:
            return done
        job = self.prepare_clip(
            image, lambda h, w: self.check_inputs(image, h, w), height=height, width=width, num_frames=num_frames,
            decode_chunk_size=decode_chunk_size, fps=fps, motion_bucket_id=motion_bucket_id,
            noise_aug_strength=noise_aug_strength, num_videos_per_prompt=num_videos_per_prompt, generator=generator,
            latents=latents, latent_channels=self.unet.config.in_channels, min_guidance_scale=min_guidance_scale,
            max_guidance_scale=max_guidance_scale, num_inference_steps=num_inference_steps)
        if bbox_images is not None:        # bbox-frame latents replace the first / last conditioning frames (:200-206)
            boxes = self._encode_vae_condition(bbox_images, job.device, num_videos_per_prompt,
                                               job.cfg).to(job.cond_latents.dtype)
            job.cond_latents[:, 0:num_cond_bbox_frames] = boxes[:, 0:num_cond_bbox_frames]
            job.cond_latents[:, -1] = boxes[:, -1]
        with self.progress_bar(total=num_inference_steps) as bar:
            out = self._denoise(job.latents, job.cond_latents, job.clip_embeds, job.time_ids, None,
                                num_inference_steps, min_guidance_scale, max_guidance_scale, 1.0,
                                callback_on_step_end, callback_on_step_end_tensor_inputs, bar, do_cfg=job.cfg)
        return self.finish_clip(job, out, output_type, return_dict, clamp=True)      # decoded frames clamped (:297)
