"""--inerf-cluster-fit (intrinsicnerf_amd/launch.py): the reference's Cluster / Cluster_Manager get the GPU
``update_center`` and the render_path mirrors build the package's Cluster_Manager; without the flag the reference's
bindings stay (test_launch_cpu.py).  Same stand-in entry scripts and subprocess as test_launch_cpu.py."""
from test_launch_cpu import PRELUDE, _run, ref  # noqa: F401  (ref: the stand-in tree fixture)

OBJECT_FIT = PRELUDE + r'''
from intrinsicnerf_amd import cluster as ic
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", with_render_path=True, cluster_fit=True)
cl = sys.modules["cluster"]
assert cl.Cluster_Manager.update_center is ic.update_center
if hasattr(cl, "Cluster"):
    assert cl.Cluster.update_center is ic.fit_cluster
assert mod.render_path.keywords["cluster_manager_factory"] is ic.Cluster_Manager
assert mod.Cluster_Manager is cl.Cluster_Manager                 # the script's own name still points at its module's class
print("object-level cluster fit ok")
'''

SSR_FIT = PRELUDE + r'''
from intrinsicnerf_amd import cluster as ic
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", with_render_path=True, cluster_fit=True)
trainer, cl = sys.modules["SSR.training.trainer"], sys.modules["SSR.training.cluster"]
assert cl.Cluster_Manager.update_center is ic.update_center and cl.Cluster_Manager.dest_color is ic.dest_color
t = trainer.SSRTrainer.__new__(trainer.SSRTrainer)
assert t.cluster_manager_factory is ic.Cluster_Manager
assert "update_center" in mod.__inerf_bound__["SSR.training.cluster.Cluster_Manager"]
print("ssr cluster fit ok")
'''

DEFAULT = PRELUDE + r'''
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", with_render_path=True)
trainer, cl = sys.modules["SSR.training.trainer"], sys.modules["SSR.training.cluster"]
assert cl.Cluster_Manager.update_center.__code__.co_filename.endswith("cluster.py")
assert not cl.Cluster_Manager.update_center.__module__.startswith("intrinsicnerf_amd")
assert trainer.SSRTrainer.__new__(trainer.SSRTrainer).cluster_manager_factory is trainer.Cluster_Manager
print("default bindings ok")
'''


def test_cluster_fit_flag_binds_object_level(ref):
    assert "object-level cluster fit ok" in _run(OBJECT_FIT, ref)


def test_cluster_fit_flag_binds_ssr(ref):
    assert "ssr cluster fit ok" in _run(SSR_FIT, ref)


def test_without_flag_the_reference_fit_stays(ref):
    assert "default bindings ok" in _run(DEFAULT, ref)


def test_flag_is_parsed_and_removed(monkeypatch):
    from intrinsicnerf_amd import launch
    seen = {}
    monkeypatch.setattr(launch, "prepare", lambda script, rp, cf: seen.update(script=script, rp=rp, cf=cf) or (type("M", (), {"__dict__": {}})(), compile("", "x", "exec")))
    import sys
    monkeypatch.setattr(sys, "argv", sys.argv[:])
    try:
        launch.main(["run_nerf.py", "--inerf-cluster-fit", "--config", "x"])
    except Exception:
        pass
    assert seen.get("cf") is True and seen.get("rp") is False
