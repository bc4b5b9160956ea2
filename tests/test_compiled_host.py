"""CPU-only checks of compiled inference: the prune_weights and compile_model commands, the compiled model file (data only), the host-side refusals of
the loader and of the test command, and the host halves of the two new library entry points."""
import pytest
import torch


def _cs():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    return CS


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """A stage-3 weights file, its pruned form and the compiled model file written from that."""
    from dualsuperreslearningforsemseg_amd.command_handlers.compile_model import compile_model
    from dualsuperreslearningforsemseg_amd.command_handlers.prune_weights import prune_weights
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    d = tmp_path_factory.mktemp('compiled')
    torch.manual_seed(7)
    stage3 = DSRL(3, _cs()).eval()
    sd3 = stage3.state_dict()
    src, pruned, compiled = str(d / 'stage3.weights'), str(d / 'sub' / 'pruned.weights'), str(d / 'model.compiled')
    torch.save({'model_state_dict': sd3, 'mixed_precision': 'O0', 'amp_state_dict': None}, src)
    dataset = {'settings': _cs()}
    prune_weights(src, pruned, dataset)
    compile_model(pruned, compiled, dataset, batch_size=2, model_input_size=(64, 128), conv_precision='f16x1')
    return {'sd3': sd3, 'src': src, 'pruned': pruned, 'compiled': compiled, 'dataset': dataset}


def test_prune_weights_keeps_exactly_the_stage1_keys(files):
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    out = torch.load(files['pruned'], map_location='cpu')
    assert set(out) == {'model_state_dict', 'mixed_precision', 'amp_state_dict'}
    assert out['mixed_precision'] == 'O0' and out['amp_state_dict'] is None
    want = DSRL(1, _cs()).state_dict()
    got = out['model_state_dict']
    assert list(got) == list(want)
    assert len(got) < len(files['sd3']) and any(k.startswith('SISR_decoder') for k in files['sd3']) and not any(k.startswith('SISR') for k in got)
    for k, v in got.items():
        assert v.dtype == files['sd3'][k].dtype and torch.equal(v, files['sd3'][k]), k


def test_compile_model_refuses_unpruned_and_names_prune_weights(files, tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.compile_model import compile_model
    with pytest.raises(RuntimeError, match='prune_weights'):
        compile_model(files['src'], str(tmp_path / 'x.compiled'), files['dataset'])
    assert not (tmp_path / 'x.compiled').exists()


def test_compiled_file_is_data_only_with_the_documented_fields(files):
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.compile_model import compile_model
    CS = _cs()
    d = torch.load(files['compiled'], map_location='cpu', weights_only=True)         # no code, no pickled classes of this package
    assert d['format'] == 'dsrl-hip-compiled' and d['format_version'] == 1 and d['abi_version'] == _lib.load().dsrl_version()
    assert d['model_input_size'] == [64, 128] and d['batch_size'] == 2 and d['conv_precision'] == 'f16x1'
    assert d['NUM_CLASSES'] == CS.NUM_CLASSES and d['IGNORE_CLASS_LABEL'] == CS.IGNORE_CLASS_LABEL
    assert d['MEAN'] == [float(v) for v in CS.MEAN] and d['STD'] == [float(v) for v in CS.STD]
    assert d['CLASS_RGB_COLOR'] == {int(k): [int(c) for c in v] for k, v in CS.CLASS_RGB_COLOR.items()}
    assert all(type(v) is list for v in d['CLASS_RGB_COLOR'].values()) and type(d['MEAN']) is list
    pruned = torch.load(files['pruned'], map_location='cpu')['model_state_dict']
    assert list(d['model_state_dict']) == list(pruned)
    for k, v in d['model_state_dict'].items():
        assert torch.equal(v, pruned[k]), k
    # the defaults: batch size 1, the project's input size, the current conv arithmetic
    out = files['compiled'] + '.default'
    compile_model(files['pruned'], out, files['dataset'])
    e = torch.load(out, map_location='cpu', weights_only=True)
    from dualsuperreslearningforsemseg_amd import settings
    assert e['batch_size'] == 1 and tuple(e['model_input_size']) == tuple(settings.MODEL_INPUT_SIZE) and e['conv_precision'] == HF.get_conv_precision()


def test_loader_refuses_wrong_versions_and_plain_files_on_the_host(files, tmp_path):
    from dualsuperreslearningforsemseg_amd.inference import load_compiled_model, read_compiled_file
    good = torch.load(files['compiled'], map_location='cpu', weights_only=True)
    assert read_compiled_file(files['compiled'])['format_version'] == 1
    for field, value in (('format_version', 2), ('abi_version', good['abi_version'] + 1)):
        bad = str(tmp_path / (field + '.compiled'))
        torch.save(dict(good, **{field: value}), bad)
        with pytest.raises(RuntimeError, match=field):
            read_compiled_file(bad)
        with pytest.raises(RuntimeError, match=field):             # the loader itself: refused before any device work (there is no device here)
            load_compiled_model(bad, torch.device('cuda', 0))
    with pytest.raises(RuntimeError, match='compile_model'):        # a plain weights file names the command that writes compiled files
        read_compiled_file(files['pruned'])
    with pytest.raises(RuntimeError, match='compile_model'):
        read_compiled_file(str(tmp_path / 'missing.compiled'))


def test_commands_on_other_devices_and_mixed_up_files(files, tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import NOT_GPU, benchmark, load_eval_model
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    import re
    with pytest.raises(RuntimeError, match=re.escape(NOT_GPU)):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), files['compiled'], 'cpu', True)
    with pytest.raises(RuntimeError, match=re.escape(NOT_GPU)):
        benchmark(files['compiled'], dict(files['dataset'], split='val'), 'cpu', 0, 2, compiled_model=True)
    # a plain weights file with compiled_model=True: refused on the host, naming the other command
    with pytest.raises(RuntimeError, match='compile_model'):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), files['pruned'], 'gpu', True)
    # a compiled file read as plain weights: refused before the model reaches a device, naming the flag
    with pytest.raises(RuntimeError, match='compiled_model=True'):
        load_eval_model(files['compiled'], _cs(), torch.device('cpu'))


def test_new_entry_points_are_exported_and_check_their_arguments_on_the_host():
    from dualsuperreslearningforsemseg_amd import _lib
    import dualsuperreslearningforsemseg_amd as D
    for name in ('dsrl_class_map_visualize', 'dsrl_fingerprint_segments', 'dsrl_fingerprint_segment_words'):
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.dsrl_fingerprint_segment_words() == 32768
    a = 1 << 20
    assert lib.dsrl_class_map_visualize(None, a, None, a, a, 1, 4, 4, 255, 0.4, None) == -1            # null image
    assert lib.dsrl_class_map_visualize(a, a, None, a, a, 1, 4, 4, 255, 1.0, None) == -1               # blend factor outside (0, 1)
    assert lib.dsrl_class_map_visualize(a, a, None, a, a, 1, 4, 4, 256, 0.4, None) == -1               # ignore label outside a byte
    assert lib.dsrl_class_map_visualize(a, a, None, a, a, 64, 2048, 2048, 255, 0.4, None) == -2        # beyond the 32-bit index
    assert b'32 bits' in lib.dsrl_last_error()
    assert lib.dsrl_fingerprint_segments(None, 1, a, None, None, 0, None) == -1
    assert lib.dsrl_fingerprint_segments(a, 1, None, None, None, 0, None) == -1                        # neither an output nor (expect, flag)
    assert D.CompiledPredictor is D.inference.CompiledPredictor and hasattr(D.DSRL, 'compile_predict')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.functional.class_map_visualize(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(256, 3, dtype=torch.uint8))
