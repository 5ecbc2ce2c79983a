"""The network object the evaluation code drives -- the slice of
``mdir/learning/network.py`` that inference needs.

``extract_vectors`` receives this wrapper, not an ``nn.Module``
(``cirscore.py:54`` -> ``network.py:88-89``): it must offer ``.eval()``,
``.meta['out_channels']``, ``.model`` and ``__call__(image) = wrappers[stage](image,
model)``.  ``SingleNetwork`` / ``CirNetwork`` keep the reference's constructor,
``overlay_params`` and checkpoint layout (``{"type","frozen","network_params":{"model",
"runtime"},"model_state"}``, network.py:142-170).  Training-side methods
(parameters, freeze, graphs) are out of scope.  ``SequentialNetwork`` is the inference slice of ``network.py:204-345``: a U-Net
generator (``unet.py``) in front of the embedding network, one checkpoint.
"""
import copy
from collections import namedtuple

import torch

from .networks import init_network
from .unet import MODEL_LABELS as UNET_LABELS
from .wrapper import initialize_wrappers


def init_cirnet(**params):
    """``mdir/components/model/network/cirnet.py:10-22`` minus the model-zoo download.  ``precision`` ("f32" / "f16", optional)
    passes through to ``init_network``."""
    for key in ["local_whitening", "pooling", "regional", "whitening", "pretrained"]:
        if key not in params:
            raise ValueError("Key '%s' not in params" % key)
    params["mean"] = [0.485, 0.456, 0.406]
    params["std"] = [0.229, 0.224, 0.225]
    params["architecture"] = params.pop("cir_architecture")
    net = init_network(params)
    net.meta["in_channels"] = 3
    net.meta["out_channels"] = net.meta["outputdim"]
    return net


MODEL_LABELS = {"cirnet": init_cirnet, **UNET_LABELS}


def initialize_model(params):
    return MODEL_LABELS[params.pop("architecture")](**params)


class SingleNetwork:
    TRAIN, EVAL = "train", "eval"
    NetworkParams = namedtuple("NetworkParams", ["model", "runtime"])

    def __init__(self, model, network_params, device, frozen):
        self.meta = {"in_channels": model.meta["in_channels"], "out_channels": model.meta["out_channels"]}
        self.network_params = network_params
        wrappers = network_params.runtime.get("wrappers", "")
        if isinstance(wrappers, dict):
            assert wrappers.keys() == {"train", "eval"}, wrappers.keys()
            self.wrappers = {x: initialize_wrappers(wrappers[x], device) for x in wrappers}
        else:
            self.wrappers = {x: initialize_wrappers(wrappers, device) for x in ["train", "eval"]}
        self.frozen = network_params.runtime.get("frozen", False) or frozen
        if "precision" in network_params.runtime:          # scenarios/eval_f16_trunk.yml: the labelled fp16 trunk of networks.py
            model.set_precision(network_params.runtime["precision"])
        self.model = model.to(device)
        self.stage = None
        if self.frozen:
            self.eval()
        extra = network_params.runtime.keys() - {"data", "wrappers", "frozen", "precision"}
        assert not extra, extra
        extra = network_params.runtime.get("data", {}).keys() - {"mean_std", "transforms"}
        assert not extra, extra

    supports_batches = True          # the wrapper chain answers one row per image for a batch (wrapper.Compose)

    def __call__(self, image):
        return self.wrappers[self.stage](image, self.model)

    def eval(self):
        self.model.eval()
        self.stage = self.EVAL
        return self

    def overlay_params(self, new_params, device):
        if not new_params:
            return self
        new_params["runtime"]["frozen"] = True
        network_params = self.NetworkParams(self.network_params.model, new_params.pop("runtime"))
        assert not new_params
        return self.__class__(self.model, network_params, device, frozen=True)

    def state_dict(self):
        return {"net": {"type": self.__class__.__name__, "frozen": self.frozen,
                        "network_params": self.network_params._asdict(),
                        "model_state": self.model.state_dict()}}

    @classmethod
    def initialize_from_state(cls, state_dict, device, params, runtime):
        assert state_dict.keys() == {"net"}, state_dict.keys()
        checkpoint = state_dict["net"]
        assert checkpoint.keys() == {"type", "frozen", "network_params", "model_state"}, checkpoint.keys()
        network_params = cls.NetworkParams(**checkpoint["network_params"])
        assert checkpoint["type"] == cls.__name__, checkpoint["type"]
        model = initialize_model(copy.deepcopy(network_params.model))
        model.load_state_dict(checkpoint["model_state"])
        if runtime:
            network_params.runtime.update(runtime)
        return cls(model, network_params, device=device, frozen=checkpoint["frozen"])


class CirNetwork(SingleNetwork):
    def __init__(self, model, network_params, device, frozen):
        data = network_params.runtime.setdefault("data", {})
        if "mean_std" not in data:
            data["mean_std"] = [model.meta["mean"], model.meta["std"]]
        super().__init__(model, network_params, device, frozen)


class SequentialNetwork:
    """Member networks run one after the other: ``sequence = [first, last]``, the first a generator whose output the last
    embeds.  The pre- and post-processing chain of the whole is the LAST network's (its own is emptied), the data section the
    FIRST's; ``model`` is the last network's, which is what the wrappers ask for pooling exponent and descriptor width."""
    TRAIN, EVAL = "train", "eval"
    NetworkParams = namedtuple("NetworkParams", ["runtime"])

    def __init__(self, networks, sequence, device, frozen):
        assert len(networks) == len(sequence) == 2, (len(networks), sequence)      # as the reference: pairs only
        self.sequence = sequence
        self.networks = networks
        first, last = networks[sequence[0]], networks[sequence[1]]
        # every refusal before anything is taken from a member: a failed construction leaves the members as they were
        for net in networks.values():
            if net.network_params.runtime.get("precision", "f32") != "f32":
                raise NotImplementedError("precision: %s on a SequentialNetwork: the generators run in fp32 only"
                                          % net.network_params.runtime["precision"])
        if first.meta["in_channels"] != 3:
            raise NotImplementedError("a first network with in_channels=%s: the multi-channel input transforms (tospace, "
                                      "add_clahe_fromrgb, replace_histogram) are out of scope" % first.meta["in_channels"])
        assert first.meta["out_channels"] == last.meta["in_channels"], (first.meta, last.meta)
        self.frozen = frozen
        self.model = last.model
        self.stage = None
        self.wrappers = last.wrappers
        last.wrappers = {x: initialize_wrappers("", device) for x in ["train", "eval"]}
        self.network_params = self.NetworkParams({"wrappers": last.network_params.runtime.get("wrappers", ""),
                                                  "data": first.network_params.runtime.get("data", {})})
        self.meta = {"in_channels": first.meta["in_channels"], "out_channels": last.meta["out_channels"]}
        if frozen:
            self.eval()

    @property
    def supports_batches(self):
        """A batch goes through the members' models directly (``forward``); a member with a chain of its own is called as a
        network, one image at a time."""
        return all(not self.networks[net].wrappers[self.stage or self.EVAL].wrappers for net in self.sequence)

    def __call__(self, image):
        return self.wrappers[self.stage](image, self.forward, self.model)

    def __getitem__(self, key):
        return self.networks[key]

    def forward(self, image):
        for name in self.sequence:
            net = self.networks[name]
            # an empty chain is `model(image.to(device))`; calling the model keeps a batch's [D,B] as the outer chain expects it
            image = net(image) if net.wrappers[net.stage].wrappers else net.model(image)
        return image

    def eval(self):
        for net in self.sequence:
            self.networks[net].eval()
        self.stage = self.EVAL
        return self

    def overlay_params(self, new_params, device):
        if not new_params:
            return self
        diff = set(self.sequence) - set(new_params.keys())
        assert not diff, diff
        # a last member without an overlay of its own keeps the chain of the pair, which lives here (its own was emptied)
        acc = {}
        for net in self.sequence:
            acc[net] = self.networks[net].overlay_params(new_params[net], device)
            if acc[net] is self.networks[net] and net == self.sequence[-1]:
                acc[net] = copy.copy(acc[net])
                acc[net].wrappers = self.wrappers
        return self.__class__(acc, self.sequence, device=device, frozen=True)

    def state_dict(self):
        hierarchy, state = {}, {}
        for net in self.sequence:
            netstate = self.networks[net].state_dict()
            netstate[net] = netstate.pop("net")
            overlap = set(state.keys()).intersection(netstate.keys())
            assert not overlap, overlap
            hierarchy[net] = [x for x in netstate if x != net]
            state.update(netstate)
        state["net"] = {"type": self.__class__.__name__, "frozen": self.frozen, "sequence": self.sequence,
                        "network_hierarchy": hierarchy}
        return state

    @classmethod
    def initialize_from_state(cls, state_dict, device, params, runtime):
        state_dict = dict(state_dict)
        checkpoint = state_dict.pop("net")
        assert checkpoint["type"] == cls.__name__, checkpoint["type"]
        if not {"sequence", "network_hierarchy"} <= checkpoint.keys():
            raise NotImplementedError("not a complete SequentialNetwork checkpoint: %s lacks 'sequence' / 'network_hierarchy' "
                                      "(a SequentialNetwork = U-Net generator + embedding network, DESIGN.md section 7)"
                                      % sorted(checkpoint.keys()))
        assert checkpoint.keys() == {"type", "frozen", "sequence", "network_hierarchy"}, checkpoint.keys()
        assert set(checkpoint["sequence"]) == checkpoint["network_hierarchy"].keys()
        runtime = dict(runtime) if runtime else {}
        if runtime.pop("precision", "f32") != "f32":                  # f32 is what a sequence runs in: nothing to pass on
            raise NotImplementedError("precision: f16 on a SequentialNetwork: the generators run in fp32 only")
        propagated = {net: None for net in checkpoint["sequence"]}
        if "wrappers" in runtime:
            propagated[checkpoint["sequence"][-1]] = {"wrappers": runtime.pop("wrappers")}
        if "data" in runtime:
            first = checkpoint["sequence"][0]
            propagated[first] = {**(propagated[first] or {}), "data": runtime.pop("data")}
        assert not runtime, runtime
        acc = {}
        for net in checkpoint["network_hierarchy"]:
            netstate = {x: state_dict[x] for x in checkpoint["network_hierarchy"][net]}
            netstate["net"] = state_dict[net]
            acc[net] = NETWORKS[state_dict[net]["type"]].initialize_from_state(netstate, device, None, propagated[net])
        return cls(acc, checkpoint["sequence"], device=device, frozen=checkpoint["frozen"])


NETWORKS = {"SingleNetwork": SingleNetwork, "CirNetwork": CirNetwork, "SequentialNetwork": SequentialNetwork}


def load_checkpoint(path):
    """``Checkpoints.load_network`` for a single file (mdir/learning/checkpoints.py:145-155)."""
    from .scenario import open_resource
    checkpoint = torch.load(open_resource(path), map_location="cpu", weights_only=False)
    assert "net" not in checkpoint.get("_networks_included", {})
    return {"net": checkpoint, **checkpoint.pop("_networks_included", {})}


def initialize_network(params, device, state=None, runtime=None):
    assert state is not None, "only checkpoint-backed networks are supported on the eval path"
    kind = state["net"]["type"]
    if kind not in NETWORKS:
        raise NotImplementedError("network type %r is outside the MI355X hot path (%s are supported, DESIGN.md section 7)"
                                  % (kind, sorted(NETWORKS)))
    cls = NETWORKS[kind]
    if cls is SequentialNetwork:                        # its member networks are further top-level entries of the checkpoint
        return cls.initialize_from_state(state, device, params, runtime)
    return cls.initialize_from_state({"net": state["net"]}, device, params, runtime)


def load_network(params, device):
    """``mdir/learning/__init__.py:9-11``: ``{"path": <.pth>, "runtime": <overrides>}``."""
    return initialize_network(None, device, load_checkpoint(params["path"]), params["runtime"])
