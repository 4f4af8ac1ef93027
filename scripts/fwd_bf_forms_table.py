"""profiles/fwd_bf_forms_parity.txt from a parity log (tests/conftest.py parity_log: the file SSC_PARITY_LOG names, or its
default): per case and process of tests/test_gpu_fwd_bf16_forms.py, the child processes' launches included, the plan and the
worst err / bound ratio of its launches (mid: a K range begins in the middle of a tap row / parity class; red4: slabs summed by
slab_reduce4_kernel 1, slab_reduce_kernel 0, no slabs -1).
python scripts/fwd_bf_forms_table.py <parity.jsonl> > <table>"""
import json
import sys

recs = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
recs = [r for r in recs if r['test'] == 'fwd_bf16_forms']
worst = {}
for r in recs:
    c = r['config']
    key = (c['case'], c.get('child', '-'), c['corun'], tuple(r['plan']))
    if key not in worst or r['ratio'] > worst[key]['ratio']:
        worst[key] = r
print('%-28s %-5s %-5s %-4s %-3s  %-6s %-4s %-5s %-3s %-2s %-6s %-6s %5s %5s %6s %-3s %-4s %5s  %-9s %-9s %-9s' %
      ('case', 'child', 'corun', 'nk', 'acc', 'kernel', 'tile', 'plain', 'src', 'SS', 'korder', 'layout', 'slabs', 'whole', 'slices', 'mid', 'red4', 'K',
       'err/bound', 'err', 'bound'))
for (case, child, corun, p), r in worst.items():
    c = r['config']
    print('%-28s %-5s %-5d %-4d %-3d  %-6s %-4d %-5d %-3d %-2d %-6d %-6d %5d %5d %6d %-3d %-4d %5d  %.3e %.3e %.3e' %
          (case, child, corun, c['bmode'], c['accumulate'], 'bfh' if p[0] else 'bf', p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9],
           c['mid_start'], c['reduce4'], r['K'], r['ratio'], r['max_abs_err'], r['bound']))
for k, name in ((0, 'conv_bf_kernel'), (1, 'conv_bfh_kernel')):
    mine = [r for r in worst.values() if r['plan'][0] == k]
    if mine:
        w = max(mine, key=lambda r: r['ratio'])
        print('%s: %d lines, worst err/bound %.3e (%s)' % (name, len(mine), w['ratio'], w['config']['case']))
