"""Drop-in boundary: ``install_aliases()`` makes the reference's top-level import names resolve to this repository.

Two cases, each in a fresh interpreter:
* a user's ``dataManagement`` package is importable (the reference's tree on ``sys.path``): only its leaf
  ``myTransforms`` is swapped, so the user's ``dataModules`` / ``myDatasets`` stay theirs and their
  ``from .myTransforms import MyTransform`` picks up the device transform.  The test writes a stand-in tree of that shape
  (placeholder classes, plus ``models`` / ``trainingModules`` / ``myTransforms`` modules that fail if they are ever
  imported instead of the aliases);
* no such package: the alias package provides ``dataManagement.myTransforms`` itself."""
import os
import subprocess
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SHADOWED = "raise ImportError('stand-in {} imported: install_aliases() did not take')\n"
STANDIN_TREE = {
    "dataManagement/__init__.py": "",
    "dataManagement/myDatasets.py": "class StandInDataset:\n    pass\n",
    "dataManagement/dataModules.py": ("from .myDatasets import StandInDataset\nfrom .myTransforms import MyTransform\n\n\n"
                                      "class StandInDataModule:\n    pass\n"),
    "dataManagement/myTransforms.py": _SHADOWED.format("dataManagement.myTransforms"),
    "models/__init__.py": _SHADOWED.format("models"),
    "trainingModules/__init__.py": _SHADOWED.format("trainingModules"),
}

DRIVER = textwrap.dedent(r'''
    import sys

    STANDIN, REPO = sys.argv[1], sys.argv[2]
    sys.path.insert(0, REPO)
    sys.path.insert(0, STANDIN)

    import sim2real_lane_segment_amd as amd
    amd.install_aliases()
    ours = "sim2real_lane_segment_amd."

    from trainingModules.SimpleTrain import SimpleTrainModule, RightLaneModule
    from trainingModules.MMETrainingModule import MMETrainingModule
    from trainingModules.TrainingBase import TrainingBase
    from dataManagement.myTransforms import MyTransform
    for cls in (SimpleTrainModule, MMETrainingModule, TrainingBase, MyTransform):
        assert cls.__module__.startswith(ours), cls.__module__

    # the user's dataManagement package stays theirs; its relative import of myTransforms gets the device transform
    import dataManagement, dataManagement.dataModules as dm, dataManagement.myDatasets as ds
    for mod in (dataManagement, dm, ds):
        assert mod.__file__.startswith(STANDIN), mod.__file__
    assert dm.StandInDataModule.__module__ == "dataManagement.dataModules"
    assert dm.StandInDataset is ds.StandInDataset
    assert dm.MyTransform is MyTransform

    # models.* incl. the legacy EncDecNet resolve through the alias
    from models.EncDecNet import EncDecNet, Conv, activationTypes
    from models.FCDenseNet.tiramisu import (FCDenseNet, FCDenseNet57, FCDenseNet67, FCDenseNet103, FCDenseNet57Base,
                                            FCDenseNet57Classifier, FCDenseNet67Base, FCDenseNet67Classifier,
                                            FCDenseNetFeatureExtractor, FCDenseNetClassifier, grad_reverse)
    import models.EncDecNet, models.FCDenseNet.layers
    assert EncDecNet.__module__.startswith(ours) and FCDenseNet57.__module__.startswith(ours)
    assert models.EncDecNet.EncDecNet is EncDecNet
    assert RightLaneModule is SimpleTrainModule
    m = SimpleTrainModule(lr=1e-3, lrRatio=1000, decay=1e-4, num_cls=4)
    assert len(m.state_dict()) == 434
    print("ALIAS-OK")
''')


def test_reference_scripts_import_through_aliases(tmp_path):
    for rel, src in STANDIN_TREE.items():
        path = tmp_path / "standin" / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(src)
    script = tmp_path / "alias_driver.py"
    script.write_text(DRIVER)
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "standin"), REPO], capture_output=True, text=True,
                       timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALIAS-OK" in r.stdout


def test_aliases_without_reference_on_path(tmp_path):
    """Without rightLaneNetwork/ on sys.path the alias package still offers dataManagement.myTransforms."""
    code = ("import sys; sys.path.insert(0, %r); import sim2real_lane_segment_amd as a; a.install_aliases();"
            "from dataManagement.myTransforms import MyTransform; from models.EncDecNet import EncDecNet;"
            "from trainingModules.SimpleTrain import SimpleTrainModule; print('OK')" % REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
