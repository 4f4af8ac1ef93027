"""profiles/wgrad_forms_parity.txt from a parity log (tests/conftest.py parity_log: the file SSC_PARITY_LOG names, or its default):
one line per launch of tests/test_gpu_wgrad_forms.py.  python scripts/wgrad_forms_table.py <parity.jsonl> > <table>"""
import json
import sys

recs = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
recs = [r for r in recs if r['test'] == 'wgrad_forms']
print('%-28s %-6s %-3s %-6s %-7s %5s %-4s %-10s %5s  %-9s %-9s %-9s' %
      ('case', 'ws', 'acc', 'pinned', 'tile', 'split', 'view', 'reduce', 'K', 'err/bound', 'err', 'bound'))
for r in recs:
    c = r['config']
    print('%-28s %-6s %-3d %-6s %-7s %5d %-4s %-10s %5d  %.3e %.3e %.3e' %
          (c['case'], c['ws'], c['accumulate'], 'cfg0' if 'pinned' in c else '-', c['tile'], c['split'], c['view'], c['reduce'],
           r['K'], r['ratio'], r['max_abs_err'], r['bound']))
print('%d launches, worst err/bound %.3e' % (len(recs), max(r['ratio'] for r in recs)))
