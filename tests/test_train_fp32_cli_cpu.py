"""`--coder-fp32` of tdvc_amd.tools.train and the `coder_fp32` argument of TrainStep, without touching a device."""
import inspect


def test_coder_fp32_flag_parses():
    from tdvc_amd.tools.train import make_parser
    ap = make_parser()
    assert ap.parse_args([]).coder_fp32 is False
    a = ap.parse_args(["--coder-fp32", "--iters", "3"])
    assert a.coder_fp32 is True and a.iters == 3


def test_train_step_signature_accepts_coder_fp32():
    from tdvc_amd.train import TrainStep
    p = inspect.signature(TrainStep.__init__).parameters
    assert "coder_fp32" in p and p["coder_fp32"].default is False
    assert p["distortion"].default == "mse" and p["graph"].default is False          # the neighbours keep their defaults


def test_model_attribute_defaults_off():
    from tdvc_amd.model.pnet import VideoCompressor
    m = VideoCompressor()
    assert m.train_coder_fp32 is False and m.coder_fp32 is False
