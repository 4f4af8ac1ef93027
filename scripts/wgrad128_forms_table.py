"""profiles/wgrad128_forms_parity.txt from a parity log (tests/conftest.py parity_log: the file SSC_PARITY_LOG names, or its
default): one line per launch of tests/test_gpu_wgrad128_forms.py, the child process's launches included.
python scripts/wgrad128_forms_table.py <parity.jsonl> > <table>"""
import json
import sys

recs = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
recs = [r for r in recs if r['test'] == 'wgrad128_forms']
print('%-24s %-6s %-6s %-3s %-5s  %-3s %-6s %-5s %5s %-3s %-2s %6s  %-9s %-9s %-9s' %
      ('case', 'arith', 'ws', 'acc', 'child', 'TPT', 'gplain', 'dense', 'split', 'xcd', 'DB', 'K', 'err/bound', 'err', 'bound'))
for r in recs:
    c, p = r['config'], r['plan']
    assert p[0] == (1 if c['arith'] == 'bf16x6' else 0), r
    print('%-24s %-6s %-6s %-3d %-5s  %-3d %-6d %-5d %5d %-3d %-2d %6d  %.3e %.3e %.3e' %
          (c['case'], c['arith'], c['ws'], c['accumulate'], 'yes' if 'child' in c else '-', p[1], p[2], p[3], p[4], p[5], p[6],
           r['K'], r['ratio'], r['max_abs_err'], r['bound']))
for a in ('exact', 'bf16x6'):
    mine = [r for r in recs if r['config']['arith'] == a]
    if mine:
        w = max(mine, key=lambda r: r['ratio'])
        print('%s: %d launches, worst err/bound %.3e (%s)' % (a, len(mine), w['ratio'], w['config']['case']))
