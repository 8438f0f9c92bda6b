#!/usr/bin/env python3
"""Cost of the camera gradients at BASELINE configs[3] (1 M Gaussians, 1080p), one view, map frozen:
   (a) tracking iteration: forward + L1 loss + backward with ONLY the camera twist as a leaf (gsr_backward_camera) + Adam on it;
   (b) the same iteration with the plain backward of a call whose Gaussians require grad (no camera gradient), for comparison.
With --rgbd, three RGB-D tracking iterations (loss 0.5 L1(colour) + 0.5 mean|(D_z - gt_depth) valid|, valid = gt_depth > 0 and
A > 0.5, as scene_utils.refine_pose forms it):
   (c) photometric only (= (a));
   (d) RGB-D in ONE pass: render(depth="z", alpha=True);
   (e) RGB-D through the two-render workaround: the colour render, then a second full rasterization with colors_precomp =
       (z, 0, 0) and bg = (0, 1, 0) - channel 0 is D_z, channel 1 is T_final - z formed with torch from the pose's viewmatrix.
With --device-pose, the same iterations with the pose on the device, as scene_utils.track_pose runs them (DevicePoseCamera,
gsr_pose_forward / gsr_pose_backward with the Adam step folded in, forward_mode="exact"):
   (f) photometric, render(camera_only=True): the track_pose iteration;
   (g) the same with the full camera backward (camera_only off): what the camera-only backward alone is worth;
   (h) (with --rgbd) RGB-D in one pass, camera_only=True.
Every form is also timed as a LOOP (`*_loop_ms`: the iterations back to back, one synchronisation at the end, per iteration): the
device forms never wait for the host inside the loop, which the per-iteration timing (a synchronisation after each) cannot show.
Prints one JSON line (ms per iteration, medians of timed repetitions).  Per-kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/camera_grad_bench.py` and read preprocess_bwd vs its camera form and cam_reduce.
    python tools/camera_grad_bench.py [--iters N] [--rgbd] [--device-pose]   (GPU box, repo root)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rgbd", action="store_true", help="also time the RGB-D tracking iterations (c) - (e)")
    ap.add_argument("--device-pose", action="store_true", help="also time the track_pose-style iterations (f) - (h)")
    a = ap.parse_args()
    from scene_utils import make_config, GaussianModel, PoseCamera, l1_loss
    from gaussian_renderer import render, PipelineParams
    dev = "cuda"
    raw, cams, cfg = make_config(3, views=2)
    cam = cams[0].to(dev)
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    frozen = GaussianModel.from_raw(raw.to(dev), requires_grad=False)
    trained = GaussianModel.from_raw(raw.to(dev), requires_grad=True)
    with torch.no_grad():
        gt = render(cams[1].to(dev), frozen, pipe, bg)["render"].clone()
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu")        # as refine_pose builds it
    opt = torch.optim.Adam([pc.tau], lr=1e-4)

    def tracking():
        opt.zero_grad(set_to_none=True)
        l1_loss(render(pc, frozen, pipe, bg)["render"], gt).backward()
        opt.step()

    def plain():
        for p in trained.parameters():
            p.grad = None
        l1_loss(render(cam, trained, pipe, bg)["render"], gt).backward()

    fns = [("tracking_iter_ms", tracking), ("plain_train_bwd_iter_ms", plain)]
    if a.rgbd:
        from fused_ssim import l1_mean_loss
        with torch.no_grad():
            gt_depth = render(cams[1].to(dev), frozen, pipe, bg, depth="z")["depth"].clone()
        has = gt_depth > 0
        aux_bg = torch.tensor([0.0, 1.0, 0.0], device=dev)

        def rgbd_one_pass():
            opt.zero_grad(set_to_none=True)
            pkg = render(pc, frozen, pipe, bg, depth="z", alpha=True)
            valid = (has & (pkg["alpha"].detach() > 0.5)).float()
            (0.5 * l1_loss(pkg["render"], gt) + l1_mean_loss(pkg["depth"], gt_depth, 0.5, valid)).backward()
            opt.step()

        def rgbd_two_render():
            opt.zero_grad(set_to_none=True)
            image = render(pc, frozen, pipe, bg)["render"]
            V = pc.world_view_transform.to(dev, torch.float32)
            z = frozen.get_xyz @ V[:3, 2] + V[3, 2]
            aux_col = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], dim=1)
            aux = render(pc, frozen, pipe, aux_bg, override_color=aux_col)["render"]
            D, A = aux[0:1], 1.0 - aux[1:2]
            valid = (has & (A.detach() > 0.5)).float()
            (0.5 * l1_loss(image, gt) + l1_mean_loss(D.contiguous(), gt_depth, 0.5, valid)).backward()
            opt.step()

        fns += [("rgbd_one_pass_iter_ms", rgbd_one_pass), ("rgbd_two_render_iter_ms", rgbd_two_render)]
    if a.device_pose:
        from scene_utils import DevicePoseCamera
        from scene_utils.pose import _pose_adam_state
        dpc = DevicePoseCamera(cam, device=dev)
        dpc._adam = _pose_adam_state(dev, 1e-4, 1.0)       # the Adam step rides in gsr_pose_backward, as in track_pose

        def device_tracking(camera_only=True):
            l1_loss(render(dpc, frozen, pipe, bg, camera_only=camera_only, forward_mode="exact")["render"], gt).backward()

        fns += [("device_pose_iter_ms", device_tracking),
                ("device_pose_full_backward_iter_ms", lambda: device_tracking(False))]
        if a.rgbd:
            def device_rgbd():
                pkg = render(dpc, frozen, pipe, bg, depth="z", alpha=True, camera_only=True, forward_mode="exact")
                valid = (has & (pkg["alpha"].detach() > 0.5)).float()
                (0.5 * l1_loss(pkg["render"], gt) + l1_mean_loss(pkg["depth"], gt_depth, 0.5, valid)).backward()

            fns.append(("device_pose_rgbd_iter_ms", device_rgbd))
    out = {"config": 3, "P": cfg["P"], "W": cfg["W"], "H": cfg["H"]}
    for name, fn in fns:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = round(ts[len(ts) // 2], 4)
        # the same iterations back to back: three loops of `iters`, the median loop, per iteration
        loops = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            loops.append(e0.elapsed_time(e1) / a.iters)
        loops.sort()
        out[name.replace("_iter_ms", "_loop_ms")] = round(loops[1], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
