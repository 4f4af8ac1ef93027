"""Child process of tests/test_gpu_train_validation.py (helper, not a test module): obj_colorization_main.py with everything that
a run draws at random pinned, so that two runs of one command give the same weights bit for bit -- the training queues get fixed
seeds (the command line seeds them from the system on one GPU) and torch's generators, which draw the generator's noise
vectors, are seeded.  After the run it prints what the record caches of the process hold:

    CHILD_CACHES [{"dir": ..., "records": ..., "sk": true|false, "skf": true|false, "size": ..., "device": ...}, ...] <builds>

    python tests/train_validation_child.py <the arguments of obj_colorization_main.py>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    import torch
    import obj_colorization_main as cli
    from sketchyscenecolorization_amd import record_cache as rc
    from sketchyscenecolorization_amd.obj_lib import main_procedure as mp

    base = mp.RecordQueue

    class SeededQueue(base):
        def __init__(self, batch_size, small, which, data_base_dir='data', seed=None, record_cache=None):
            base.__init__(self, batch_size, small, which, data_base_dir=data_base_dir, seed=4000 + which,
                          record_cache=record_cache)

    mp.RecordQueue = SeededQueue
    torch.manual_seed(7)
    cli.main(list(argv))
    torch.cuda.synchronize()
    caches = [{'dir': k[0], 'records': len(c), 'sk': c.sk is not None, 'skf': c.skf is not None, 'size': c.size,
               'device': str(c.device)} for k, c in rc._MEMO.items()]
    print('CHILD_CACHES %s %d' % (json.dumps(caches), rc.BUILDS))


if __name__ == '__main__':
    main(sys.argv[1:])
