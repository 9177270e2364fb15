"""Shared by the frame-assembly tests (test_tall_frames_gpu.py, test_multi_assembly_gpu.py): the
Cornell box seen from its own camera position (main.rs:417-512) at any width and height with
square pixels, so that frames a few pixels wide or a few rows high can be as tall or as wide as
the assembly code's edges need and still cost next to nothing. The vertical field of view is 37
degrees, not the scene's 40: at 40 the first and last rows of a tall strip look past the box's
ceiling and floor (800 tan 20 = 291 > 278) into the black background, and a black row written
to the wrong place cannot be told from a black row. TEST INFRASTRUCTURE ONLY."""
import surely_rt as rt

VFOV = 37.0  # 800 tan 18.5 = 268 < 278: every row of a strip sees the inside of the box


def strip_camera(W: int, H: int, sqrt_spp: int, depth: int = 8) -> rt.RtCamera:
    """Camera::new at aspect W / H; the aspect is nudged when (int)(W / aspect) loses a row."""
    for aspect in (W / H, W / (H + 0.25), W / (H + 0.5)):
        cam = rt.camera_new(aspect, W, sqrt_spp * sqrt_spp, depth, VFOV, (278.0, 278.0, -800.0),
                            (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 0.0, 0.0, (0.0, 0.0, 0.0))
        if cam.image_height == H:
            break
    assert cam.image_height == H and cam.image_width == W and cam.sqrt_spp == sqrt_spp
    assert cam.max_depth == depth
    return cam


def cornell_blob():
    blob, _ = rt.preset_blob("cornell_box", width=8, spp=1)
    return blob
