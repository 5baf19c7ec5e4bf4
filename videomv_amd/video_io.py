"""The file writers that the entrances and the 3-D export (gs_export.py) share: the reference's frame PNGs / mp4 and the PNG contact sheet."""
import logging
import os

import torch


def _save_frames_safe(local_path, video, cfg):
    try:                                            # (inference_text2video_entrance.py:296-300: errors are logged, not raised)
        save_video_frames(local_path, video, cfg.mean, cfg.std)
        logging.info('Save video to dir %s:' % local_path)
    except Exception as e:
        logging.info(f'Step: save text or video error with {e}')


def save_video_frames(local_path, gen_video, mean, std, save_fps=8):
    """The reference writer's outputs (utils/video_op.py:166-211, ``save_i2vgen_video_safe``) as far as this image allows:
    the de-normalised frames ``clamp(v * std + mean, 0, 1) * 255`` truncated to uint8, one PNG per view named
    ``<local_path minus .mp4>/{fid:05d}.png`` (written by cv2 in the reference, PIL here: same pixels), and
    ``<local_path>`` itself — an H.264 mp4 at ``save_fps`` — when an encoder exists (``imageio`` with ffmpeg, or an ``ffmpeg``
    binary on PATH; neither ships in this image, in which case only the PNGs are written and the fact is logged).
    A single-frame video becomes ``<local_path>.png`` as in the reference.  Returns the list of files written."""
    import shutil
    import subprocess
    import numpy as np
    from PIL import Image
    v = gen_video.detach().float().cpu()
    v = v * torch.tensor(std).view(1, -1, 1, 1, 1) + torch.tensor(mean).view(1, -1, 1, 1, 1)
    v = (v.clamp(0, 1) * 255.0)[0].permute(1, 2, 3, 0)                   # f h w c  (the reference saves sample 0)
    frames = [f.numpy().astype('uint8') for f in v]                      # astype truncates, as the reference does
    written = []
    if len(frames) == 1:
        Image.fromarray(frames[0]).save(local_path + '.png')
        return [local_path + '.png']
    frame_dir = local_path.replace('.mp4', '')
    os.makedirs(frame_dir, exist_ok=True)
    for fid, frame in enumerate(frames):
        fp = os.path.join(frame_dir, '{:05d}.png'.format(fid))
        Image.fromarray(frame).save(fp)
        written.append(fp)
    try:
        import imageio                                                    # the reference's encoder
        writer = imageio.get_writer(local_path, fps=save_fps, codec='libx264', quality=8)
        for frame in frames:
            writer.append_data(frame)
        writer.close()
        written.append(local_path)
    except Exception:
        exe = shutil.which('ffmpeg')
        if exe is not None:
            cmd = [exe, '-y', '-loglevel', 'quiet', '-framerate', str(save_fps), '-start_number', '0', '-i',
                   os.path.join(frame_dir, '%05d.png'), '-vcodec', 'libx264', '-crf', '17', '-pix_fmt', 'yuv420p', local_path]
            if subprocess.run(cmd).returncode == 0:
                written.append(local_path)
        else:
            logging.info(f'no H.264 encoder in this environment (imageio / ffmpeg): wrote {len(frames)} PNG frames to {frame_dir}')
    return written


def _save_contact_sheet(video, path, mean, std):
    """video [1, 3, F, H, W] in normalised range -> one PNG with the F views side by side (best effort)."""
    try:
        from PIL import Image
        v = video[0].permute(1, 2, 3, 0).float()                     # F H W C
        v = (v * torch.tensor(std) + torch.tensor(mean)).clamp(0, 1)
        sheet = torch.cat(list(v), dim=1)                            # H, F*W, C
        Image.fromarray((sheet * 255).round().byte().numpy()).save(path)
    except Exception as e:  # pragma: no cover
        logging.info(f'Step: save png error with {e}')
