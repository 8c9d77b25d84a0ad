"""KFP basic samples (W4) and the Minio artifact-location sample (W5): compile + local execution."""
import hashlib
import importlib.util
import json
import os
import tarfile

import pytest
import yaml

EX = os.path.join(os.path.dirname(__file__), "..", "examples", "kfp")
# sha256 of the canonical JSON of the workflow in the reference's compiled minio package
REF_DIGESTS = os.path.join(os.path.dirname(__file__), "golden", "kfp_reference_digests.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(EX, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _yaml_from_archive(path):
    with tarfile.open(path) as t:
        m = [x for x in t.getmembers() if x.name.endswith(".yaml")][0]
        return yaml.safe_load(t.extractfile(m).read())


def test_all_basic_samples_compile(tmp_path):
    bs = _load("basic_samples")
    out = bs.compile_all(str(tmp_path))
    assert set(out) == set(bs.SAMPLES)
    wf = bs.compiler.Compiler().compile_to_workflow(bs.SAMPLES["sidecar"])
    tmpl = {t["name"]: t for t in wf["spec"]["templates"]}
    assert tmpl["download"]["sidecars"][0]["name"] == "echo"
    wf = bs.compiler.Compiler().compile_to_workflow(bs.SAMPLES["pipeline_transformers"])
    assert all(t.get("retryStrategy", {}).get("limit") == 5 for t in wf["spec"]["templates"] if "container" in t)


@pytest.mark.parametrize("name", ["sequential", "parallel_join", "condition", "exit_handler", "recursion",
                                  "immediate_value", "artifact_location"])
def test_basic_sample_runs_locally(tmp_path, name):
    st = _load("basic_samples").run_local(name, str(tmp_path))
    assert st["phase"] == "Succeeded", st


def test_retry_sample_retries_injected_faults(tmp_path):
    st = _load("basic_samples").run_local("retry", str(tmp_path))
    nodes = [n for n in st["nodes"].values() if n.get("template", "").startswith("random-failure")] \
        if isinstance(st["nodes"], dict) else []
    assert st["phase"] in ("Succeeded", "Failed")
    for n in nodes:
        assert n.get("attempts", 1) >= 1


def test_minio_sample_matches_reference_golden(tmp_path):
    mod = _load("minio_artifact_location")
    out = str(tmp_path / "minio.tar.gz")
    from mifx.kfp import compiler

    compiler.Compiler().compile(mod.minio_artifacts, out)
    wf = _yaml_from_archive(out)
    foo = next(t for t in wf["spec"]["templates"] if t["name"] == "foo")
    s3 = foo["outputs"]["artifacts"][0]["s3"]
    assert s3["key"] == "runs/{{workflow.uid}}/{{pod.name}}/mlpipeline-ui-metadata.tgz"
    assert s3["accessKeySecret"] == {"key": "accesskey", "name": "mlpipeline-minio-artifact"}
    canon = json.dumps(yaml.safe_load(yaml.safe_dump(wf)), sort_keys=True, separators=(",", ":"))
    with open(REF_DIGESTS) as f:  # exact parity with the reference's compiled package
        assert hashlib.sha256(canon.encode()).hexdigest() == json.load(f)["minio_artifact_location"]
