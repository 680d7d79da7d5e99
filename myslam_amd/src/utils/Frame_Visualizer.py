"""The in-loop frame visualiser (reference src/utils/Frame_Visualizer.py:43-122): every `freq` frames and `inside_freq`
iterations the current frame is rendered from the current pose and a 2 x 3 panel is written to `vis_dir`: input depth,
rendered depth, depth residual; input RGB, rendered RGB, RGB residual.

The panel is built on the device (ops.vis_panel: eslam_vis_panel) at the frame's own resolution and
downloaded once; the file is written with PIL.  What differs from the reference's figure: no 300-dpi matplotlib canvas and
no axes - one image pixel per frame pixel, the six titles drawn with PIL's built-in font into a strip above each row - and
save_imgs returns the frame's render metrics (ops.frame_metrics) where the reference returns None.
"""
import os

import torch

from ..common import cam_pose_to_matrix

TITLES = (('Input Depth', 'Generated Depth', 'Depth Residual'), ('Input RGB', 'Generated RGB', 'RGB Residual'))
TITLE_STRIP = 14            # pixel rows of the strip above each row of panels (titles=True)


class Frame_Visualizer(object):
    """
    Visualizes itermediate results, render out depth and color images.
    Args:
        freq (int): frequency of visualization (in frames).
        inside_freq (int): frequency of visualization inside one frame (in iterations).
        vis_dir (str): visualization directory.
        renderer (Renderer): renderer.
        truncation (float): truncation distance.
        verbose (bool): verbose or not.
        device (str): device.
        fmt (str): 'jpg' (quality 95) or 'png' (exact).
        titles (bool): draw the six titles into a strip above each row.
    """

    def __init__(self, freq, inside_freq, vis_dir, renderer, truncation, verbose, device='cuda:0', fmt='jpg', titles=True):
        if fmt not in ('jpg', 'png'):
            raise ValueError(f"Frame_Visualizer: fmt must be 'jpg' or 'png', got {fmt!r}")
        self.freq = freq
        self.device = device
        self.vis_dir = vis_dir
        self.verbose = verbose
        self.renderer = renderer
        self.inside_freq = inside_freq
        self.truncation = truncation
        self.fmt = fmt
        self.titles = bool(titles)
        os.makedirs(f'{vis_dir}', exist_ok=True)

    def panel_rows(self, H):
        """The pixel rows of the written image that hold the two rows of panels: (slice of row 0, slice of row 1)."""
        s = TITLE_STRIP if self.titles else 0
        return slice(s, s + H), slice(2 * s + H, 2 * s + 2 * H)

    def _with_titles(self, panel):
        """The panel (numpy uint8 [2H,3W,3]) with a white strip above each row and the titles centred over their panels."""
        import numpy as np
        from PIL import Image, ImageDraw, ImageFont
        H, W = panel.shape[0] // 2, panel.shape[1] // 3
        out = np.full((2 * (H + TITLE_STRIP), 3 * W, 3), 255, dtype=np.uint8)
        r0, r1 = self.panel_rows(H)
        out[r0] = panel[:H]
        out[r1] = panel[H:]
        img = Image.fromarray(out)
        draw = ImageDraw.Draw(img)
        font = ImageFont.load_default()
        for r, row in enumerate(TITLES):
            for c, text in enumerate(row):
                tw = draw.textlength(text, font=font)
                draw.text((c * W + max(0.0, (W - tw) / 2), r * (H + TITLE_STRIP) + 1), text, fill=(0, 0, 0), font=font)
        # (a title wider than its panel runs over its neighbour's strip; never over the panels)
        return img

    def save_imgs(self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, all_planes, decoders):
        """
        Visualization of depth and color images and save to file.
        Args:
            idx (int): current frame index.
            iter (int): the iteration number.
            gt_depth (tensor): ground truth depth image of the current frame.
            gt_color (tensor): ground truth color image of the current frame.
            c2w_or_camera_tensor (tensor): camera pose, represented in
                camera to world matrix or quaternion and translation tensor.
            all_planes (Tuple): feature planes.
            decoders (torch.nn.Module): decoders for TSDF and color.
        Returns:
            None when the gate (idx % freq == 0 and iter % inside_freq == 0) is false: nothing is touched.  Otherwise
            ops.frame_metrics of the rendered frame: dict(psnr, ssim, depth_l1, n_valid).
        """
        if not ((idx % self.freq == 0) and (iter % self.inside_freq == 0)):
            return None
        from PIL import Image
        from ... import ops
        with torch.no_grad():
            gt_depth = gt_depth.squeeze(0)
            gt_color = gt_color.squeeze(0)
            if c2w_or_camera_tensor.shape[-1] > 4:  ## 6od
                c2w = cam_pose_to_matrix(c2w_or_camera_tensor.clone().detach()).squeeze()
            else:
                c2w = c2w_or_camera_tensor.squeeze().detach()

            depth, color = self.renderer.render_img(all_planes, decoders, c2w, self.truncation,
                                                    self.device, gt_depth=gt_depth)
            stats = ops.frame_stats(depth, color, gt_depth, gt_color)
            panel = ops.vis_panel(depth, color, gt_depth, gt_color, stats=stats)
            metrics = ops.frame_metrics(depth, color, gt_depth, gt_color, stats=stats)
            panel = panel.cpu().numpy()                                  # the one download of the image

        img = self._with_titles(panel) if self.titles else Image.fromarray(panel)
        path = f'{self.vis_dir}/{idx:05d}_{iter:04d}.{self.fmt}'
        if self.fmt == 'jpg':
            img.save(path, quality=95)
        else:
            img.save(path)
        if self.verbose:
            print(f'Saved rendering visualization of color/depth image at {path}')
        return metrics
