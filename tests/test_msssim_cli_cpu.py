"""CPU: the command line and the constructor accept the MS-SSIM distortion and refuse anything else, before any GPU use."""
import pytest


def test_train_tool_parser_takes_the_distortion():
    from tdvc_amd.tools.train import make_parser
    ap = make_parser()
    assert ap.parse_args([]).distortion == "mse"
    assert ap.parse_args(["--distortion", "ms-ssim"]).distortion == "ms-ssim"
    assert ap.parse_args(["--distortion", "mse", "--batch", "2"]).distortion == "mse"
    with pytest.raises(SystemExit):
        ap.parse_args(["--distortion", "psnr"])


def test_train_step_refuses_an_unknown_distortion():
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.train import StepLog, TrainStep
    with pytest.raises(ValueError):
        TrainStep(VideoCompressor(), distortion="nonsense")
    assert "distortion" not in StepLog.KEYS and len(StepLog.KEYS) == 8


def test_pyramid_check_is_the_176_pixel_rule():
    """five levels of the 11-tap window: 176 -> 88 -> 44 -> 22 -> 11 (an odd size pools upwards, so 161 -> 81 -> 41 -> 21 -> 11 is the
    smallest side that passes, as in the reference); the check runs on the host, before any launch"""
    from tdvc_amd import metrics
    metrics._check_pyramid(176, 176, 5, 11)
    metrics._check_pyramid(177, 203, 5, 11)
    metrics._check_pyramid(161, 176, 5, 11)
    for h, w in ((160, 176), (176, 160), (128, 128)):
        with pytest.raises(ValueError):
            metrics._check_pyramid(h, w, 5, 11)
    with pytest.raises(ValueError):
        metrics._check_pyramid(64, 64, 1, 17)
