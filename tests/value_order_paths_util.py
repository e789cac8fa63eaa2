"""Shared by test_value_order_paths.py, next to value_order_util.py (whose templates, pool and pods it builds on): reviews that carry
their Namespace, pods wider than value_order_util.random_pod draws, many pairwise different values, and pods that hold given pairs of
values in a shuffled document order."""
import random

import value_order_util as U
from gatekeeper_amd import driver as D


def reviews(objs, namespaces=None):
    """value_order_util.reviews; namespaces (a list, or None): the Namespace object each review carries"""
    return [D.AugmentedUnstructured(D.Unstructured(o), namespaces[i] if namespaces else None, "Original") for i, o in enumerate(objs)]


def update_reviews(objs, namespaces=None):
    """value_order_util.update_reviews in the objects' own namespaces: each object against the next one as its oldObject (the last one
    has none: CREATE)"""
    out = []
    for i, o in enumerate(objs):
        r = {"uid": "u%d" % i, "kind": {"group": "", "version": "v1", "kind": "Pod"}, "operation": "UPDATE" if i + 1 < len(objs) else "CREATE",
             "name": o["metadata"]["name"], "namespace": o["metadata"]["namespace"], "object": o}
        if i + 1 < len(objs):
            r["oldObject"] = dict(objs[i + 1], metadata=o["metadata"])
        out.append(D.AugmentedReview(D.AdmissionRequest(r), namespaces[i] if namespaces else None, "Original"))
    return out


def random_pod(rng, name, pool=U.POOL, max_containers=8, max_ports=6):
    """value_order_util.random_pod with more room: at most eight containers of at most six ports, at most three volumes, every compared
    member now and then absent"""
    def pick(d, k):
        if rng.random() < 0.85:
            d[k] = rng.choice(pool)
    cs = []
    for ci in range(rng.randrange(0, max_containers + 1)):
        c = {"name": "c%d" % ci, "image": "i"}
        lim = {}
        pick(lim, "count")
        if rng.random() < 0.9:
            c["resources"] = {"limits": lim}
        ports = []
        for pi in range(rng.randrange(0, max_ports + 1)):
            p = {"name": rng.choice(["a", "b", "vol-long-name"])}
            pick(p, "containerPort")
            pick(p, "hostPort")
            ports.append(p)
        if ports or rng.random() < 0.5:
            c["ports"] = ports
        cs.append(c)
    extra = {}
    for k in ("minReplicas", "maxReplicas", "maxCount", "replicas"):
        pick(extra, k)
    vols = []
    for vi in range(rng.randrange(0, 4)):
        v = {"name": rng.choice(["a", "b", "vol-long-name"])}
        pick(v, "port")
        vols.append(v)
    extra["volumes"] = vols
    return U.pod(cs, name, **extra)


def namespace(name, **labels):
    return {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": name, "labels": labels}}


def in_namespaces(objs, names):
    """copies of the objects, dealt round robin into the named namespaces (the objects themselves stay as they are)"""
    return [dict(o, metadata=dict(o["metadata"], namespace=names[i % len(names)])) for i, o in enumerate(objs)]


def wide_pod(rng, name, n_containers, n_ports, pool=U.POOL, **spec_extra):
    """every container with all its ports and both compared members: more elements than a small LDS capacity holds"""
    cs = [{"name": "c%d" % ci, "image": "i", "resources": {"limits": {"count": rng.choice(pool)}},
           "ports": [{"name": rng.choice(["a", "b", "vol-long-name"]), "containerPort": rng.choice(pool), "hostPort": rng.choice(pool)} for _ in range(n_ports)]}
          for ci in range(n_containers)]
    spec_extra.setdefault("volumes", [{"name": n, "port": rng.choice(pool)} for n in ("a", "b", "vol-long-name")])
    return U.pod(cs, name, **spec_extra)


def many_values(seed, n):
    """n pairwise different values of every kind the device ranks among each other: integers, non-integral floats and strings of 3 to
    20 bytes -- half of the strings behind one 12-byte prefix, so that many of them differ only beyond a heap string's header bytes"""
    rng = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        k = rng.randrange(4)
        if k == 0:
            v = rng.randrange(-10 ** 12, 10 ** 12) if rng.random() < 0.5 else rng.randrange(-70000, 70000)
        elif k == 1:
            v = rng.randrange(-10 ** 6, 10 ** 6) + rng.choice([0.5, 0.25, 0.125, 0.75])   # (a binary fraction: never integral, exact as text)
        elif k == 2:
            v = "".join(rng.choice("abcdefghijklmnopqrstuvwxy") for _ in range(rng.randrange(3, 21)))
        else:
            v = "shared-prefx" + "".join(rng.choice("abcdefghijklmnopqrstuvwxy") for _ in range(rng.randrange(1, 9)))
        if (type(v), v) not in seen:
            seen.add((type(v), v))
            out.append(v)
    return out


def ports_pod(rng, name, pairs, n_containers, volume_ports):
    """one pod whose ports hold the (containerPort, hostPort) pairs: the ports shuffled over the containers and either member first in
    a port's text, so that the order of first occurrence in the document says nothing about the order of the values"""
    pairs = list(pairs)
    rng.shuffle(pairs)
    per = len(pairs) // n_containers
    assert per * n_containers == len(pairs)
    cs = []
    for ci in range(n_containers):
        ports = []
        for k, (cp, hp) in enumerate(pairs[ci * per:(ci + 1) * per]):
            p = {"name": "p%d" % k}
            for member, v in rng.sample([("containerPort", cp), ("hostPort", hp)], 2):
                p[member] = v
            ports.append(p)
        cs.append({"name": "c%d" % ci, "image": "i", "ports": ports})
    return U.pod(cs, name, volumes=[{"name": "v%d" % i, "port": v} for i, v in enumerate(volume_ports)])
