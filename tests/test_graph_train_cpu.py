"""--graph / --graph_warmup on the command line: parser and the refusals that fire before anything touches the GPU."""
import pytest
import torch


def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_defaults_and_flags():
    from gdn_amd import option
    a = option.parse_args(["synthetic", "--synthetic"])
    assert a.graph is False and a.graph_warmup == 3
    a = option.parse_args(["synthetic", "--synthetic", "--graph"])
    assert a.graph is True and a.graph_warmup == 3
    a = option.parse_args(["synthetic", "--synthetic", "--graph", "--graph_warmup", "1"])
    assert a.graph is True and a.graph_warmup == 1


@pytest.mark.parametrize("bad", ["0", "-2", "x"])
def test_graph_warmup_must_be_positive(bad, capsys):
    from gdn_amd import option
    with pytest.raises(SystemExit):
        option.parse_args(["synthetic", "--synthetic", "--graph", "--graph_warmup", bad])
    assert "--graph_warmup" in capsys.readouterr().err


@pytest.mark.parametrize("mode", ["DtoD_test", "RtoD_test"])
def test_graph_with_a_test_mode_is_refused_before_the_gpu(monkeypatch, mode):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = option.parse_args(["synthetic", "--synthetic", "--mode", mode, "--graph"])
    with pytest.raises(RuntimeError, match="trains nothing"):
        GDN_main.run(a)


def test_graph_with_global_berhu_on_two_ranks_is_refused_before_the_gpu(monkeypatch):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    a = option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD", "--graph", "--global_berhu"])
    with pytest.raises(RuntimeError, match="global_berhu"):
        GDN_main.run(a)
    assert not torch.distributed.is_initialized()


def test_graph_makes_the_optimizer_capturable():
    from gdn_amd import GDN_main, option
    p = [torch.nn.Parameter(torch.zeros(3))]

    class M:
        def parameters(self):
            return p
    assert GDN_main._make_optimizer(M(), option.parse_args(["synthetic", "--graph"])).capturable is True
    assert GDN_main._make_optimizer(M(), option.parse_args(["synthetic"])).capturable is False


def test_bind_outputs_checks_its_tensors():
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import GpuAugmentLoader, GpuCropLoader, GpuNYUAugmentLoader, GpuResidentLoader, SyntheticRawKitti
    loader = GpuAugmentLoader(SyntheticRawKitti(4, 8, 16), 2, "cpu", train=False)
    gt, rgb = torch.zeros(2, 1, 8, 16), torch.zeros(2, 3, 8, 16)
    loader.bind_outputs(gt, rgb, gt.clone())
    assert loader._outs(2)[0] is gt and loader._outs(1) is None
    loader.bind_outputs(gt, None, None)
    assert loader._outs(2) == (gt, None, None)
    loader.bind_outputs(None, None, None)
    assert loader._outs(2) is None
    with pytest.raises(GdnError, match="different sizes"):
        loader.bind_outputs(gt, torch.zeros(3, 3, 8, 16), None)
    with pytest.raises(GdnError):
        loader.bind_outputs(gt.double(), None, None)
    assert GpuResidentLoader.bind_outputs is GpuAugmentLoader.bind_outputs
    assert GpuCropLoader.bind_outputs is None and GpuNYUAugmentLoader.bind_outputs is None      # these keep the copy
