"""ibl.trainers has the reference's public surface — read from the reference's source with `ast`, nothing of it is
imported or executed — and its host-side decisions (train_layers from the model, loss_type, vlad=False, the parsing of
a loader batch) hold without a GPU."""
import ast
import inspect
import os

import pytest
import torch

REFERENCE = "/root/reference/ibl/trainers.py"


@pytest.mark.skipif(not os.path.isfile(REFERENCE), reason="the reference tree is only present in the build container")
def test_public_surface_of_the_reference_trainers_is_present():
    import ibl.trainers as ours
    tree = ast.parse(open(REFERENCE).read())
    problems, classes = [], 0
    for node in tree.body:
        if not isinstance(node, (ast.FunctionDef, ast.ClassDef)) or node.name.startswith("_"):
            continue
        if not hasattr(ours, node.name):
            problems.append(f"ibl.trainers.{node.name} missing")
            continue
        obj = getattr(ours, node.name)
        classes += isinstance(node, ast.ClassDef)
        # the trainers' underscore methods are what the reference's own scripts and the goldens call: checked as well
        items = [(node.name, node, obj)] if isinstance(node, ast.FunctionDef) else \
            [(f"{node.name}.{m.name}", m, getattr(obj, m.name, None)) for m in node.body if isinstance(m, ast.FunctionDef)]
        for label, fn, target in items:
            if target is None:
                problems.append(f"ibl.trainers.{label} missing")
                continue
            have = inspect.signature(target).parameters
            want = [a.arg for a in fn.args.args if a.arg != "self"]
            lacking = [a for a in want if a not in have]
            if lacking:
                problems.append(f"ibl.trainers.{label} lacks parameters {lacking}")
            elif [a for a in have if a in want] != want and label.split(".")[-1] in ("__init__", "train"):
                problems.append(f"ibl.trainers.{label}: parameter order {list(have)} != {want}")
            n_dflt = len(fn.args.defaults)
            for a, d in zip(want[len(want) - n_dflt:], fn.args.defaults):
                if a in have and isinstance(d, ast.Constant) and have[a].default != d.value:
                    problems.append(f"ibl.trainers.{label}: default of {a} is {have[a].default!r}, not {d.value!r}")
    assert classes == 2 and not problems, "\n".join(problems)


def test_the_package_exports_the_trainers():
    import ibl
    from ibl.trainers import SFRSTrainer, Trainer
    assert ibl.trainers.Trainer is Trainer and ibl.trainers.SFRSTrainer is SFRSTrainer
    t = Trainer(None)
    assert (t.margin, t.gpu, t.temp) == (0.3, None, 0.07)
    s = SFRSTrainer(None, None)
    assert (s.margin, s.neg_num, s.gpu, s.temp) == (0.3, 10, None, [0.07])


class _Base(torch.nn.Module):
    def __init__(self, train_layers):
        super().__init__()
        self.train_layers = train_layers
        self.conv = torch.nn.Conv2d(3, 4, 3)


class _Net(torch.nn.Module):
    def __init__(self, train_layers="conv5"):
        super().__init__()
        self.base_model = _Base(train_layers)
        self.net_vlad = torch.nn.Linear(4, 4)
        self.calls = []

    def forward_train(self, x, train_layers=None):
        self.calls.append(train_layers)
        raise RuntimeError("stop here")


class _Container(torch.nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


def test_train_layers_come_from_the_model_and_a_container_is_unwrapped():
    from ibl.trainers import SFRSTrainer, Trainer
    x = torch.zeros((1, 4, 3, 8, 8))
    for wrap in (lambda m: m, _Container):
        for layers in ("conv5", "conv4", "full"):
            net = _Net(layers)
            with pytest.raises(RuntimeError, match="stop here"):
                Trainer(wrap(net))._forward(x, True, "triplet")
            assert net.calls == [layers]
            for p in net.base_model.parameters():
                p.requires_grad_(False)
            with pytest.raises(RuntimeError, match="stop here"):
                SFRSTrainer(wrap(net), wrap(_Net()), neg_num=2)._forward(x, x[:, :3], "sare_ind", 0)
            assert net.calls == [layers, None]                  # nothing of the backbone trains: the frozen path


def test_unknown_loss_types_and_max_pooled_training_raise():
    from ibl.trainers import SFRSTrainer, Trainer
    x = torch.zeros((1, 4, 3, 8, 8))
    t, s = Trainer(_Net()), SFRSTrainer(_Net(), _Net(), neg_num=2)
    with pytest.raises(NotImplementedError, match="carries no autograd graph"):
        t._forward(x, False, "triplet")
    for call in (lambda: t._get_loss(torch.zeros((4, 8)), "hinge", 1, 4),
                 lambda: t.train(0, 0, None, None, 1, loss_type="sare"),
                 lambda: s._get_loss(torch.zeros((1, 8)), torch.zeros((1, 8)), torch.zeros((1, 2, 8)), 1, "Triplet"),
                 lambda: s._get_hard_loss(torch.zeros(8), torch.zeros(8), torch.zeros((2, 9, 8)), torch.zeros((2, 9)), ""),
                 lambda: s._forward(x, x, "softmax", 0),
                 lambda: s.train(0, 0, 0, None, None, 1, loss_type=None)):
        with pytest.raises(ValueError, match="loss_type"):
            call()
    assert not t.model.calls and not s.model.calls               # refused before the model runs


def test_parse_data_stacks_a_loader_batch():
    from ibl.trainers import SFRSTrainer
    B, neg_num, n_diff = 2, 3, 2
    batch = [(torch.full((B, 3, 4, 4), float(j)), ["name"] * B) for j in range(2 + neg_num + n_diff)]
    imgs = torch.stack([b[0] for b in batch]).permute(1, 0, 2, 3, 4)
    assert imgs.shape == (B, 7, 3, 4, 4)
    s = SFRSTrainer(None, None, neg_num=neg_num)
    arg = torch.tensor([[[0.1, 0.9, 0.3] + [0.0] * 6, [0.5] + [0.0] * 7 + [0.7]]])
    assert s.hard_regions(arg).tolist() == [[1, 8]]
    if torch.cuda.is_available():
        easy, diff = s._parse_data(batch)
        assert easy.shape == (B, 2 + neg_num, 3, 4, 4) and diff.shape == (B, 1 + n_diff, 3, 4, 4)
        assert easy[0, :, 0, 0, 0].tolist() == [0, 1, 2, 3, 4] and diff[1, :, 0, 0, 0].tolist() == [0, 5, 6]
